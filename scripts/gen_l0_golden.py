"""Record tests/golden/l0.npz from the reference package's LinearL0 / LinearLASSO (cplxmodule/nn/relevance/extensions/
real/ell_zero.py, lasso.py) on the CPU, in float32.

    python scripts/gen_l0_golden.py <reference checkout>     (the directory that holds cplxmodule/ and VERSION)

Per case (three L0 groups, the LinearL0(I, 1) shape dispatch, LASSO): input, parameters, the uniform draws of the
training forward (torch.rand / rand_like recorded while the reference runs), train and eval outputs with every gradient
(x, weight, bias, log_alpha), the elementwise penalty and the gradient of its sum, soft and hard relevance, sparsity
counts; the state dict's keys in order.  Plus the first 20 Adam steps of each phase of the reference's real-l0 and
real-lasso tracks (tests/test_relevance.py:167-185) at a small size, with the binarize -> load -> deploy hand-offs and
the final masks, as oracle/gen_golden.py:gen_trajectory records the VD tracks.  TEST INFRASTRUCTURE only.
"""
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "l0.npz")


def import_reference(ref):
    sys.path.insert(0, ref)
    m = types.ModuleType("cplxmodule.__version__")           # (a setup.py-generated module in the reference)
    m.__version__ = open(os.path.join(ref, "VERSION")).read().strip()
    sys.modules["cplxmodule.__version__"] = m
    import cplxmodule  # noqa: F401


def npy(t):
    return t.detach().cpu().numpy().copy()


class Recorder:
    """Patches torch.rand / torch.rand_like (the reference's only sources of u) and keeps every draw."""

    def __init__(self):
        self.tape = []

    def __enter__(self):
        self.rand, self.rand_like = torch.rand, torch.rand_like

        def rand(*a, **k):
            t = self.rand(*a, **k)
            self.tape.append(npy(t))
            return t

        def rand_like(x, **k):
            t = self.rand_like(x, **k)
            self.tape.append(npy(t))
            return t
        torch.rand, torch.rand_like = rand, rand_like
        return self

    def __exit__(self, *exc):
        torch.rand, torch.rand_like = self.rand, self.rand_like
        return False


# name: (class, in, out, group, input lead shape)
CASES = OrderedDict([
    ("none", ("L0", 20, 12, None, (6,))),
    ("input", ("L0", 24, 12, "input", (2, 3))),
    ("output", ("L0", 20, 16, "output", (2, 3))),
    ("dispatch", ("L0", 20, 1, None, (5,))),           # LinearL0(I, 1): log_alpha [1, I] -> the input branch
    ("lasso", ("LASSO", 20, 12, None, (6,))),
])
LASSO_THRESHOLD = float(np.log(0.25) - np.log(0.75))


def gen_cases(d):
    from cplxmodule.nn.relevance import LinearL0, LinearLASSO
    for name, (cls, I, O, group, lead) in CASES.items():
        torch.manual_seed(7)
        layer = LinearL0(I, O, group=group) if cls == "L0" else LinearLASSO(I, O)
        k = name + "_"
        d[k + "sd_keys"] = np.array(list(layer.state_dict().keys()))
        for kk, v in layer.state_dict().items():
            d[k + "sd_" + kk] = npy(v)                        # as constructed (log_alpha = -2.197)
        with torch.no_grad():
            layer.weight.uniform_(-1.0, 1.0)
            if cls == "L0":
                layer.log_alpha.uniform_(-4.0, 4.0)           # gates spread over (0, 1), some clamped at 0 or 1
            else:
                layer.weight[0, :3] = 0.0                     # |w| at 0: torch.abs's gradient is 0 there
        x = torch.randn(*lead, I)
        gy = torch.randn(*lead, O)
        d[k + "x"], d[k + "gy"] = npy(x), npy(gy)
        for kk, v in layer.named_parameters():
            d[k + "p_" + kk] = npy(v)
        for phase in ("train", "eval"):
            layer.train(phase == "train")
            layer.zero_grad()
            xg = x.clone().requires_grad_(True)
            with Recorder() as rec:
                y = layer(xg)
            (y * gy).sum().backward()
            d[k + phase + "_y"] = npy(y)
            d[k + phase + "_dx"] = npy(xg.grad)
            for kk, v in layer.named_parameters():
                d[k + phase + "_d" + kk] = npy(v.grad)
            if phase == "train" and cls == "L0":
                assert len(rec.tape) == 1
                d[k + "u"] = rec.tape[0]
        layer.zero_grad()
        pen = layer.penalty
        d[k + "penalty"] = npy(pen)
        pen.sum().backward()
        p = layer.log_alpha if cls == "L0" else layer.weight
        d[k + "penalty_grad"] = npy(p.grad)
        if cls == "L0":
            for hard in (False, True):
                tag = "hard" if hard else "soft"
                d[k + "relevance_" + tag] = npy(layer.relevance(hard=hard))
                d[k + "sparsity_" + tag] = np.array(layer.sparsity(hard=hard)[0][1])
        else:
            d[k + "relevance"] = npy(layer.relevance(threshold=LASSO_THRESHOLD))
            d[k + "sparsity"] = np.array(layer.sparsity(threshold=LASSO_THRESHOLD)[0][1])
    d["lasso_threshold"] = np.array(LASSO_THRESHOLD)


def gen_trajectories(d):
    import warnings
    import torch.nn.functional as F
    from cplxmodule.nn import masked
    from cplxmodule.nn import relevance as rel
    from cplxmodule.nn.utils.sparsity import sparsity
    warnings.simplefilter("ignore")
    N_STEPS, B, NF, NH, NO = 20, 32, 24, 10, 8

    def build(cls):
        return torch.nn.Sequential(OrderedDict([
            ("l1", cls(NF, NH, bias=True)), ("act", torch.nn.LeakyReLU()), ("l2", cls(NH, NO, bias=False))]))

    # tests/test_relevance.py:167-185 (klw and reduction per track), :198-201 (tau)
    tracks = {
        "l0": ([torch.nn.Linear, rel.LinearL0, masked.LinearMasked], [0.0, 2e-2, 0.0], "sum", 0.73105),
        "lasso": ([torch.nn.Linear, rel.LinearLASSO, masked.LinearMasked], [0.0, 1e-1, 0.0], "mean", 0.25),
    }
    for tname, (layers, klws, reduction, tau) in tracks.items():
        threshold = float(np.log(tau) - np.log(1 - tau))
        d[f"traj_{tname}_threshold"] = np.array(threshold)
        d[f"traj_{tname}_reduction"] = np.array(reduction)
        torch.manual_seed(1234)
        X = torch.randn(B, NF)
        y = -X[:, :NO].clone()
        d[f"traj_{tname}_X"], d[f"traj_{tname}_y"] = npy(X), npy(y)
        prev = None
        for ph, (cls, klw) in enumerate(zip(layers, klws)):
            torch.manual_seed(100 + ph)
            model = build(cls)
            k = f"traj_{tname}_p{ph}_"
            if prev is not None:
                state_dict = prev.state_dict()
                masks = rel.compute_ard_masks(prev, hard=False, threshold=threshold)
                state_dict, masks = masked.binarize_masks(state_dict, masks)
                model.load_state_dict(state_dict, strict=False)
                model = masked.deploy_masks(model, state_dict=masks)
                for kk, v in masks.items():
                    d[k + "deploy_" + kk] = npy(v)
            if ph == 1:
                # start the sparsification phase from a spread of relevances so that the masks are not trivial
                with torch.no_grad():
                    for m in model.modules():
                        if hasattr(m, "log_alpha"):
                            m.log_alpha.uniform_(-3.0, 4.0)
                        elif isinstance(m, torch.nn.Linear):
                            m.weight.uniform_(-1.0, 1.0)
            for kk, v in model.state_dict().items():
                d[k + "init_" + kk] = npy(v)
            model.train()
            optim = torch.optim.Adam(model.parameters())
            rows = []
            with Recorder() as rec:
                for _ in range(N_STEPS):
                    optim.zero_grad()
                    y_pred = model(X)
                    mse = F.mse_loss(y_pred, y)
                    kl_d = sum(rel.penalties(model, reduction=reduction))
                    loss = mse + klw * kl_d
                    loss.backward()
                    optim.step()
                    f_sp = sparsity(model, hard=True, threshold=threshold)
                    rows.append([float(loss), float(mse), float(kl_d), float(f_sp)])
            d[k + "traj"] = np.array(rows, dtype=np.float64)
            d[k + "klw"] = np.array(klw)
            d[k + "n_tape"] = np.array(len(rec.tape))
            for j, t in enumerate(rec.tape):
                d[k + f"tape_{j:03d}"] = t
            for kk, v in model.state_dict().items():
                d[k + "final_" + kk] = npy(v)
            for hard in (False, True):
                fm = rel.compute_ard_masks(model, hard=hard, threshold=threshold)
                for kk, v in fm.items():
                    d[k + ("finalhard_" if hard else "finalmask_") + kk] = npy(v)
            prev = model


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import_reference(os.path.abspath(sys.argv[1]))
    torch.set_num_threads(1)
    d = {}
    gen_cases(d)
    gen_trajectories(d)
    total = sum(np.asarray(v).nbytes for v in d.values())
    assert total < (1 << 20), f"{total} bytes: split the fixture (tests/conftest.py:load_golden reads parts)"
    np.savez_compressed(OUT, **d)
    print(f"l0: {len(d)} arrays, {total / 1024:.1f} KiB uncompressed, {os.path.getsize(OUT) / 1024:.1f} KiB on disk")


if __name__ == "__main__":
    main()
