"""LinearL0 / LinearLASSO on the GPU: parity with the reference (tests/golden/l0.npz, scripts/gen_l0_golden.py) with
its recorded uniforms as the tape, the reference's real-l0 / real-lasso tracks replayed step by step, bf16 against a
float64 restatement, the uniform stream against oracle/philox.py, the gate regenerated in the backward, deterministic
per-column reductions, hipGraph replays, and one headline-sized step."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from gpu_util import DEV, N, T

pytestmark = pytest.mark.gpu

CASES = {
    "none": ("L0", 20, 12, None, (6,)), "input": ("L0", 24, 12, "input", (2, 3)),
    "output": ("L0", 20, 16, "output", (2, 3)), "dispatch": ("L0", 20, 1, None, (5,)),
    "lasso": ("LASSO", 20, 12, None, (6,)),
}
BETA, GAMMA, ZETA = 0.66, -0.1, 1.1


def _close(got, ref, tol=1e-5, what=""):
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * max(float(np.abs(ref).max()), 1e-30), err_msg=what)


@pytest.fixture
def noise_mode():
    from cplxmodule_amd.nn.relevance import noise
    prev = noise.mode
    yield noise
    noise._tape = []
    noise.set_mode(prev)


def _layer(cfg, g=None, k=None):
    from cplxmodule_amd.nn.relevance import LinearL0, LinearLASSO
    cls, I, O, group, _ = cfg
    layer = (LinearL0(I, O, group=group) if cls == "L0" else LinearLASSO(I, O)).to(DEV)
    if g is not None:
        layer.load_state_dict({n: T(g[k + "p_" + n]) for n, _ in layer.named_parameters()})
    return layer


@pytest.mark.parametrize("name", list(CASES))
def test_golden_parity(golden, noise_mode, name):
    g = golden("l0")
    k = name + "_"
    cfg = CASES[name]
    layer = _layer(cfg, g, k)
    for phase in ("train", "eval"):
        layer.train(phase == "train")
        layer.zero_grad(set_to_none=True)
        if phase == "train" and cfg[0] == "L0":
            noise_mode.set_tape([torch.from_numpy(g[k + "u"])])
        x = T(g[k + "x"]).requires_grad_(True)
        y = layer(x)
        (y * T(g[k + "gy"])).sum().backward()
        assert not getattr(noise_mode, "_tape", None)
        _close(N(y), g[k + phase + "_y"], what=f"{name} {phase} y")
        _close(N(x.grad), g[k + phase + "_dx"], what=f"{name} {phase} dx")
        for n, p in layer.named_parameters():
            _close(N(p.grad), g[k + phase + "_d" + n], what=f"{name} {phase} d{n}")
    layer.zero_grad(set_to_none=True)
    pen = layer.penalty
    _close(N(pen), g[k + "penalty"], what="penalty")
    pen.sum().backward()
    p = layer.log_alpha if cfg[0] == "L0" else layer.weight
    _close(N(p.grad), g[k + "penalty_grad"], what="penalty gradient")
    from cplxmodule_amd.nn.relevance import penalties
    for red in ("sum", "mean"):
        tot = sum(penalties(layer, reduction=red))
        ref = g[k + "penalty"].sum() / (1 if red == "sum" else g[k + "penalty"].size)
        np.testing.assert_allclose(float(tot), ref, rtol=1e-5)
    if cfg[0] == "L0":
        soft, hard = layer.relevance(hard=False), layer.relevance(hard=True)
        assert soft.shape == layer.weight.shape and soft.dtype == torch.float32
        np.testing.assert_allclose(N(soft), g[k + "relevance_soft"], rtol=1e-6, atol=1e-7)
        np.testing.assert_array_equal(N(hard), g[k + "relevance_hard"])
        assert layer.sparsity(hard=True)[0][1] == float(g[k + "sparsity_hard"])
        np.testing.assert_allclose(layer.sparsity(hard=False)[0][1], float(g[k + "sparsity_soft"]), rtol=1e-5)
    else:
        tau = float(g["lasso_threshold"])
        mask = layer.relevance(threshold=tau)
        assert mask.dtype == torch.bool
        np.testing.assert_array_equal(mask.cpu().numpy(), g[k + "relevance"])
        assert layer.sparsity(threshold=tau)[0][1] == float(g[k + "sparsity"])


@pytest.mark.parametrize("track", ["l0", "lasso"])
def test_trajectory_matches_reference(golden, noise_mode, track):
    import torch.nn.functional as F
    from cplxmodule_amd.nn import masked, relevance as rel
    from cplxmodule_amd.nn.utils.sparsity import sparsity
    g = golden("l0")
    kt = f"traj_{track}_"
    threshold, reduction = float(g[kt + "threshold"]), str(g[kt + "reduction"])
    X, y = T(g[kt + "X"]), T(g[kt + "y"])
    layers = {1: rel.LinearL0 if track == "l0" else rel.LinearLASSO, 2: masked.LinearMasked}
    for ph, cls in layers.items():
        k = f"{kt}p{ph}_"
        model = torch.nn.Sequential(OrderedDict([("l1", cls(24, 10, bias=True)), ("act", torch.nn.LeakyReLU()),
                                                 ("l2", cls(10, 8, bias=False))])).to(DEV)
        model.load_state_dict({n[len(k) + 5:]: T(v) for n, v in g.items() if n.startswith(k + "init_")}, strict=True)
        if ph == 2:
            for n, m in masked.named_masks(model):
                np.testing.assert_array_equal(N(m), g[k + "deploy_" + n + ".mask"])
        noise_mode.set_tape([torch.from_numpy(g[k + f"tape_{j:03d}"]) for j in range(int(g[k + "n_tape"]))])
        klw = float(g[k + "klw"])
        model.train()
        optim = torch.optim.Adam(model.parameters())
        rows = []
        for _ in range(g[k + "traj"].shape[0]):
            optim.zero_grad()
            mse = F.mse_loss(model(X), y)
            kl_d = sum(rel.penalties(model, reduction=reduction))
            loss = mse + klw * kl_d
            loss.backward()
            optim.step()
            rows.append([float(loss), float(mse), float(kl_d), float(sparsity(model, hard=True, threshold=threshold))])
        assert not noise_mode._tape, "the whole reference tape must have been consumed"
        rows, ref = np.array(rows), g[k + "traj"]
        np.testing.assert_allclose(rows[:, :3], ref[:, :3], rtol=1e-5, atol=1e-7, err_msg=f"{track} phase {ph}")
        np.testing.assert_array_equal(rows[:, 3], ref[:, 3], err_msg=f"{track} phase {ph}: sparsity")
        for hard, tag in ((True, "finalhard_"), (False, "finalmask_")):
            for n, m in rel.compute_ard_masks(model, hard=hard, threshold=threshold).items():
                if hard or m.dtype == torch.bool or track == "lasso":
                    np.testing.assert_array_equal(N(m), g[k + tag + n], err_msg=f"final mask {n}")
                else:
                    np.testing.assert_allclose(N(m), g[k + tag + n], rtol=1e-5, atol=1e-6, err_msg=f"final mask {n}")
        for n, v in model.state_dict().items():
            refv = g[k + "final_" + n]
            np.testing.assert_allclose(N(v), refv, rtol=2e-4, atol=2e-6 * max(1.0, np.abs(refv).max()), err_msg=n)


# ---- float64 restatement of ell_zero.py ----------------------------------------------------------------------------
def _gate64(la, u=None):
    if u is None:
        s = 1 / (1 + np.exp(la))
    else:
        s = 1 / (1 + np.exp(-((np.log(u) - np.log1p(-u) - la) / BETA)))
    pre = (ZETA - GAMMA) * s + GAMMA
    dz = np.where((pre >= 0) & (pre <= 1), (ZETA - GAMMA) * s * (1 - s) * (-1 / BETA if u is not None else -1), 0)
    return np.clip(pre, 0, 1), dz


def _ref64(group, x, w, b, la, u, gy):
    """y and every gradient in float64 (x: [B, I], u in the reference layout)."""
    if group == "input":
        z, dz = _gate64(la.reshape(1, -1), u.reshape(x.shape))
        xz = x * z
        y = xz @ w.T + b
        dxz = gy @ w
        return y, {"x": dxz * z, "weight": gy.T @ xz, "bias": gy.sum(0), "log_alpha": (dxz * x * dz).sum(0)[None]}
    if group == "output":
        pre = x @ w.T
        z, dz = _gate64(la.reshape(1, -1), u.reshape(pre.shape))
        y = pre * z + b
        dpre = gy * z
        return y, {"x": dpre @ w, "weight": dpre.T @ x, "bias": gy.sum(0), "log_alpha": (gy * pre * dz).sum(0)[:, None]}
    z, dz = _gate64(la, u)
    y = x @ (w * z).T + b
    D = gy.T @ x
    return y, {"x": gy @ (w * z), "weight": D * z, "bias": gy.sum(0), "log_alpha": D * w * dz}


@pytest.mark.parametrize("group", [None, "input", "output"])
def test_bf16_against_float64(noise_mode, group):
    from cplxmodule_amd.nn.relevance import LinearL0
    torch.manual_seed(5)
    B, I, O = 96, 64, 48
    layer = LinearL0(I, O, group=group).to(DEV)
    with torch.no_grad():
        layer.log_alpha.uniform_(-4, 4)
    shape = {None: (O, I), "input": (B, 1, I), "output": (B, O, 1)}[group]
    u = torch.rand(*shape)
    noise_mode.set_tape([u])
    x = torch.randn(B, I, device=DEV).bfloat16().requires_grad_(True)
    gy = torch.randn(B, O, device=DEV).bfloat16()
    y = layer(x)
    assert y.dtype == torch.bfloat16
    y.backward(gy)
    f = lambda t: N(t).astype(np.float64)  # noqa: E731
    yr, grads = _ref64(group, f(x), f(layer.weight), f(layer.bias), f(layer.log_alpha), u.numpy().astype(np.float64),
                       f(gy))
    # the gated operand and the output are rounded to bf16 (2^-8 relative each); float32 accumulation otherwise
    _close(f(y), yr, tol=2 ** -7, what="y")
    _close(f(x.grad), grads["x"], tol=2 ** -7, what="dx")
    for n, p in layer.named_parameters():
        _close(f(p.grad), grads[n], tol=2 ** -7, what=f"d{n}")


def test_uniform_stream_matches_oracle():
    from oracle import philox
    from cplxmodule_amd import l0
    for n, seed, offset in ((1, 0, 1), (1027, 0x123456789ABCDEF, 7), (4096 * 3 + 5, 2 ** 64 - 1, 2 ** 40 + 3)):
        got = N(l0.philox_uniform(n, seed, offset, DEV))
        x = philox.philox4x32(np.arange((n + 3) // 4, dtype=np.uint64), offset, seed)
        ref = philox._u01(x).reshape(-1)[:n].astype(np.float32)
        np.testing.assert_array_equal(got, ref)
        assert got.min() > 0 and got.max() <= 1


@pytest.mark.parametrize("group", [None, "input", "output"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_backward_regenerates_the_forward_gate(noise_mode, group, dtype):
    """Philox mode (nothing kept between the passes) == tape mode fed the same uniforms, bit for bit."""
    from cplxmodule_amd import l0
    from cplxmodule_amd.nn.relevance import LinearL0
    torch.manual_seed(9)
    B, I, O = 40, 72, 56
    layer = LinearL0(I, O, group=group).to(DEV)
    with torch.no_grad():
        layer.log_alpha.uniform_(-4, 4)
    x0 = torch.randn(B, I, device=DEV).to(dtype)
    gy = torch.randn(B, O, device=DEV).to(dtype)
    shape = {None: (O, I), "input": (B, 1, I), "output": (B, O, 1)}[group]
    results = []
    for mode in ("philox", "tape"):
        noise_mode.manual_seed(1234)
        if mode == "philox":
            noise_mode.set_mode("philox")
        else:
            u = l0.philox_uniform(int(np.prod(shape)), noise_mode.seed, 1, DEV).view(shape)
            noise_mode.set_tape([u.cpu()])
        layer.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = layer(x)
        y.backward(gy)
        results.append([y, x.grad] + [p.grad for p in layer.parameters()])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_column_reduction_is_deterministic():
    from cplxmodule_amd import l0
    torch.manual_seed(2)
    for rows, cols in ((8192, 96), (3001, 37), (4096, 4096)):
        d = torch.randn(rows, cols, device=DEV)
        a = torch.randn(rows, cols, device=DEV).bfloat16()
        la = torch.empty(cols, device=DEV).uniform_(-3, 3)
        mode = l0.COLS | l0.TRAIN
        outs = [l0.gate_bwd(d, a, la, rows, cols, mode, seed=77, offset=3, da_dtype=torch.bfloat16,
                            az_dtype=torch.bfloat16)
                for _ in range(3)]
        for o in outs[1:]:
            for p, q in zip(outs[0], o):
                assert torch.equal(p, q)
        # and it is the column sum of the elementwise kernel's terms (same uniforms: the counter is the flat index)
        _, _, terms = l0.gate_bwd(d, a, la.expand(rows, cols).contiguous(), rows, cols, l0.TRAIN, seed=77, offset=3,
                                  da_dtype=torch.bfloat16, az_dtype=torch.bfloat16)
        ref = N(terms).astype(np.float64).sum(0)
        _close(N(outs[0][2]), ref, tol=1e-5, what="column sums")


def test_graph_replays_draw_fresh_gates(noise_mode):
    from cplxmodule_amd.nn import relevance as rel
    from cplxmodule_amd.utils.graphs import GraphedStep
    torch.manual_seed(3)
    noise_mode.manual_seed(21)
    noise_mode.set_mode("philox-device")
    layer = rel.LinearL0(96, 80).to(DEV)
    with torch.no_grad():
        layer.log_alpha.uniform_(-3, 3)
    x = torch.randn(32, 96, device=DEV)

    def step(xin):
        layer.zero_grad(set_to_none=True)
        y = layer(xin)
        loss = (y ** 2).sum() + 1e-2 * sum(rel.penalties(layer))
        loss.backward()
        return y, layer.log_alpha.grad, layer.weight.grad

    gs = GraphedStep(step, (x,), modules=[layer])
    state = noise_mode.device_state(torch.device(DEV))
    outs, offs = [], []
    for _ in range(2):
        offs.append(int(state[1].item()))
        res = gs.replay()
        torch.cuda.synchronize()
        outs.append([t.clone() for t in res])
    assert offs[1] == offs[0] + 1
    assert not torch.equal(outs[0][0], outs[1][0])
    noise_mode.set_mode("philox")
    for k in range(2):
        noise_mode.counter = offs[k] - 1
        got = step(x)
        for a, b in zip(got, outs[k]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("group", [None, "input", "output"])
def test_second_derivative_raises(group):
    from cplxmodule_amd.nn.relevance import LinearL0
    layer = LinearL0(16, 8, group=group).to(DEV)
    x = torch.randn(4, 16, device=DEV, requires_grad=True)
    (gx,) = torch.autograd.grad(layer(x).square().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


def test_float64_is_refused():
    from cplxmodule_amd._lib import CplxAmdError
    from cplxmodule_amd.nn.relevance import LinearL0
    layer = LinearL0(8, 4).to(DEV).double()
    with pytest.raises(CplxAmdError, match="unsupported dtype"):
        layer(torch.randn(2, 8, device=DEV, dtype=torch.float64))
    layer = LinearL0(8, 4).to(DEV)
    with pytest.raises(CplxAmdError, match="unsupported dtype"):
        layer(torch.randn(2, 8, device=DEV, dtype=torch.float64))


@pytest.mark.parametrize("group", [None, "input"])
def test_headline_size_bf16(noise_mode, group):
    """4096 -> 4096, batch 8192, bf16: forward and backward finite; sampled rows against float64 -- the first block, the
    rows on either side of the second and third trip of the gate's grid-stride loop, and the last four."""
    from cplxmodule_amd import l0
    from cplxmodule_amd.nn.relevance import LinearL0
    torch.manual_seed(11)
    B, I, O = 8192, 4096, 4096
    layer = LinearL0(I, O, group=group).to(DEV)
    with torch.no_grad():
        layer.log_alpha.uniform_(-3, 3)
    noise_mode.manual_seed(5)
    noise_mode.set_mode("philox")
    x = torch.randn(B, I, device=DEV).bfloat16().requires_grad_(True)
    gy = torch.randn(B, O, device=DEV).bfloat16()
    y = layer(x)
    y.backward(gy)
    for t in (y, x.grad, layer.weight.grad, layer.log_alpha.grad, layer.bias.grad):
        assert torch.isfinite(t.float()).all()
    rows = torch.tensor([*range(64), 1023, 1024, 1025, 2047, 2048, 2049, *range(B - 4, B)], device=DEV)
    la = layer.log_alpha.detach().double()
    if group is None:
        u = l0.philox_uniform(O * I, noise_mode.seed, 1, DEV).double().view(O, I)
        s = torch.sigmoid((torch.log(u) - torch.log1p(-u) - la) / BETA)
        wz = torch.clamp((ZETA - GAMMA) * s + GAMMA, 0, 1) * layer.weight.detach().double()
        del u, s
        yr = x[rows].detach().double() @ wz.T + layer.bias.detach().double()
        dxr = gy[rows].double() @ wz
    else:
        u = l0.philox_uniform(B * I, noise_mode.seed, 1, DEV).view(B, I)[rows].double()
        s = torch.sigmoid((torch.log(u) - torch.log1p(-u) - la) / BETA)
        z = torch.clamp((ZETA - GAMMA) * s + GAMMA, 0, 1)
        w = layer.weight.detach().double()
        yr = (x[rows].detach().double() * z) @ w.T + layer.bias.detach().double()
        dxr = (gy[rows].double() @ w) * z
    _close(N(y[rows]).astype(np.float64), yr.cpu().numpy(), tol=2 ** -7, what="y rows")
    _close(N(x.grad[rows]).astype(np.float64), dxr.cpu().numpy(), tol=2 ** -7, what="dx rows")
