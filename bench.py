"""bench.py -- Cplx-samples/sec, forward + backward (+ KL) of CplxLinearVD(4096, 4096) with bf16
activations, batch 8192 per GPU (BASELINE.json configs[1] "+ VD"), data parallel over N GPUs.

One step = zero_grad + LRT forward (complex GEMM + variance GEMM + Philox noise injection)
+ fused KL + loss (sum |y|^2 + 1e-3 KL, upstream gradient 2y) + full backward (dX, dW, db,
dlog_sigma2, dKL) [+ flat-bucket gradient all-reduce and scalar KL all-reduce for N > 1].

    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: re-executes itself under
                                                            torch.distributed.run, one rank per GPU, 127.0.0.1)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0: `metric`, `value` (samples/s), `unit`, `higher_is_better`, `dtype`, `ms_per_step`
(wall time of the K timed steps / K), `step_ms`, `config`, `kl`.  A plain run does only that: set-up, warm-up, the K
timed steps, the line.

    --full                 everything else the benchmark measures, after the timed steps: `roofline` (dominant kernel =
                           the bf16 complex MFMA GEMM, timed with HIP events in ten eager steps), `hbm_kernels_GBps`,
                           and on rank 0 with N = 1 (unless --no-cpu-baseline) the other BASELINE configurations, the
                           float32 full sizes, the data-parallel projection and `cpu_baseline` (the numpy oracle on a
                           bounded sample).  With --graph off a --full run also brackets the timed launches with HIP events.
    --dump-outputs DIR     after the timed steps, what the last timed step computed, as float32 DIR/<name>.npy (rank 0):
                           y_real / y_imag (the layer's output), x_grad_real / x_grad_imag, grad_<parameter> for every
                           parameter of the layer, kl.  Arrays of more than 2^20 elements are stored as the same fixed,
                           seeded sample of 2^20 flat positions (about 28 MB in all at the default shape).  The inputs,
                           the weights and the noise seed are fixed, so two builds run with the same arguments can be
                           compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

IN_F = OUT_F = 4096
BATCH = 8192
KLW = 1e-3
BF16_PEAK_TFLOPS = 2500.0     # MI355X dense bf16 MFMA peak, MI355X_MICROARCH.md
FP32_PEAK_TFLOPS = 157.3      # ... float32 MFMA (the 1e-5 parity mode's kernels)
HBM_PEAK_GBS = 8000.0
HBM_COPY_GBS = 6300.0         # what a plain copy reaches (same guide): anything above was not served by HBM alone


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=BATCH, help="rows per GPU")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure what the headline figure does "
                    "not need: roofline / HBM kernel figures and, with N = 1, the other configurations and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to "
                    "DIR/<name>.npy (float32; arrays above 2^20 elements as a fixed seeded sample)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: only the headline's own figures")
    ap.add_argument("--backend", default="nccl", help="nccl (= RCCL over xGMI); gloo only for "
                    "functional tests of the N > 1 path on a single GPU (with --share-device)")
    ap.add_argument("--share-device", action="store_true", help="all ranks use cuda:0 (tests)")
    ap.add_argument("--graph", choices=("on", "off"), default=os.environ.get("CPLXAMD_BENCH_GRAPH", "on"),
                    help="on (default): the step is captured ONCE in a hipGraph after the warm-up steps and every timed step is a "
                    "replay of it (same kernels, same work, fresh Philox noise per replay; with N > 1 the RCCL all-reduces "
                    "are graph nodes); off: eager launches.  A capture that fails falls back to eager.")
    ap.add_argument("--rccl-channels", type=int, default=int(os.environ.get("CPLXAMD_RCCL_MAX_CHANNELS", "0")),
                    help="cap RCCL at this many channels (= CUs its ring kernels hold while the GEMMs run; 0: RCCL's own choice); "
                    "passed to dp.init_process_group(max_channels=...)")
    ap.add_argument("--force-collectives", action="store_true", help="world of one: initialise the process group and "
                    "issue every collective of the N > 1 path anyway (tests: RCCL calls on a single-GPU box)")
    ap.add_argument("--check", action="store_true", help="after the timed region (untimed, rank 0, N = 1): value-check one "
                    "more step of exactly this workload -- as a hipGraph replay -- against float64 numpy with the numpy "
                    "Philox statement (tests/headline_check.py); the result is the line's `check` object")
    return ap.parse_args()


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it (WORLD_SIZE unset): become
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py
    <same arguments>` -- one rank per GPU; rank 0 still prints the one JSON line on this process's stdout."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    sys.stderr.flush()
    os.execv(sys.executable, cmd)


class KernelTimer:
    """HIP-event pairs around selected kernel launches, on the stream they are launched on."""

    def __init__(self):
        self.spans = {}
        self.first = {}
        self.enabled = False

    def wrap(self, mod, name, key_fn):
        inner = getattr(mod, name)

        def timed(*a, **k):
            if not self.enabled:
                return inner(*a, **k)
            key = key_fn(*a, **k)
            if key is None:
                return inner(*a, **k)
            self.first.setdefault(key, (inner, a, k))
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = inner(*a, **k)
            e.record()
            self.spans.setdefault(key, []).append((s, e))
            return out

        setattr(mod, name, timed)

    def mean_ms(self, key):
        ev = self.spans.get(key, [])
        return sum(s.elapsed_time(e) for s, e in ev) / len(ev) if ev else None

    def replay_ms(self, key, reps=10, iters=5):
        """ms per call of the FIRST timed call under `key`, re-issued `reps` times inside one hipGraph and replayed: for
        the 50-80 us HBM kernels of the step an event pair around the Python call also spans the allocation of the
        outputs and the launch gap behind them (the device idles meanwhile in an eager step); a replay does not."""
        if key not in self.first:
            return None
        inner, a, k = self.first[key]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            inner(*a, **k)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):   # (other threads: process-group watchdogs)
            for _ in range(reps):
                inner(*a, **k)
        graph.replay()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            graph.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / (iters * reps)


def cpu_baseline(sample_rows, kl_rows=512):
    """The numpy oracle (a port of the reference's op sequence) on the host cores, float32: the
    batch-proportional part (LRT forward + backward) on `sample_rows` of the 8192 rows, the
    batch-independent part (exact KL forward + backward, scipy Ei) on `kl_rows` of the 4096 weight rows;
    one full step = rows_time * (BATCH / sample_rows) + kl_time * (4096 / kl_rows).  (Both parts are linear in
    their row count; the sample keeps this leg at 1-2 s of a run whose timed region is shorter than that.)"""
    import numpy as np
    from oracle import cplx_oracle as orc
    rs = np.random.RandomState(0)
    f = np.float32
    I, O, B = IN_F, OUT_F, sample_rows
    xr, xi = rs.randn(B, I).astype(f), rs.randn(B, I).astype(f)
    bound = (1.0 / (2 * I)) ** 0.5
    wr, wi = rs.uniform(-bound, bound, (O, I)).astype(f), rs.uniform(-bound, bound, (O, I)).astype(f)
    br, bi = np.zeros(O, f), np.zeros(O, f)
    ls2 = np.full((O, I), -10, f)
    er, ei = (rs.randn(B, O) / np.sqrt(2)).astype(f), (rs.randn(B, O) / np.sqrt(2)).astype(f)
    t0 = time.perf_counter()
    yr, yi, _ = orc.lrt_cplx_linear(xr, xi, wr, wi, br, bi, ls2, er, ei)
    orc.lrt_cplx_linear_bwd(2 * yr, 2 * yi, xr, xi, wr, wi, ls2, er, ei)
    t_rows = time.perf_counter() - t0
    t0 = time.perf_counter()
    kr = min(kl_rows, O)
    kl = orc.penalty("cplx_vd", ls2[:kr], wr[:kr], wi[:kr]).sum()
    orc.penalty_bwd("cplx_vd", np.full_like(ls2[:kr], KLW), ls2[:kr], wr[:kr], wi[:kr])
    t_kl = (time.perf_counter() - t0) * (O / kr)
    assert np.isfinite(kl)
    step = t_rows * (BATCH / B) + t_kl
    return {"value": round(BATCH / step, 2), "unit": "samples/s", "cores": os.cpu_count(), "kind": "port",
            "sample": f"numpy oracle: LRT fwd+bwd on {B} of {BATCH} rows ({t_rows:.2f} s, scaled x{BATCH // B}) + the exact KL "
                      f"fwd+bwd (scipy expi) on {kr} of {O} weight rows (scaled x{O // kr}: {t_kl:.2f} s) = {step:.1f} s per step "
                      f"of {BATCH} rows"}


def gemm_traffic():
    """HBM bytes per launch of the complex GEMM from the tracked PMC summary (separate rocprofv3 --pmc passes of the
    bench's three launches at the bench shape, FETCH_SIZE doubled per the gfx950 note + WRITE_SIZE;
    scripts/r05/profile_bench.sh): (mean over the three launches, {launch: bytes}).  PMC counters cannot be read from
    inside this process, so this is the committed measurement of the same kernels and shapes, not of this run."""
    for name in ("r06_gemm_traffic.json", "r05_gemm_traffic.json", "r04_gemm_traffic.json", "r03_gemm_traffic.json", "r02_gemm_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as fh:
                d = json.load(fh)
            per = d.get("per_launch")
            if per:
                return sum(per.values()) / len(per), per
            return float(d["traffic_bytes_per_launch"]), None
        except Exception:
            continue
    return None, None


def hbm_points(dev):
    """The HBM-bound kernels at the sizes BASELINE.json quotes (rank 0, N = 1, outside the timed region):
    LRT noise injection at batch 2^20 x 2048 outputs (bf16 I/O) and the fused KL forward + backward on a
    16384 x 16384 complex weight; GB/s of ALGORITHMIC bytes, HIP events, median of 5."""
    from cplxmodule_amd import ops
    out = {}

    def med(fn, n=5):
        ts = []
        for _ in range(n + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e))
        return sorted(ts[1:])[n // 2] * 1e-3

    try:
        n = (1 << 20) * 2048
        mu_r = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        mu_i = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        s2 = torch.full((n,), 0.5, dtype=torch.float32, device=dev)
        t = med(lambda: ops.reparam_fwd(mu_r, mu_i, s2, None, 1, 2, inplace=True))
        out["reparam_fwd@2^20x2048(12B/out bf16)"] = round(12 * n / t / 1e9, 1)
        t = med(lambda: ops.reparam_bwd(mu_r, mu_i, s2, None, 1, 2, out_dtype=torch.bfloat16))
        out["reparam_bwd@2^20x2048(10B/out bf16)"] = round(10 * n / t / 1e9, 1)
        s2 = s2.bfloat16()                  # what the bf16 layers pass since r02: the variance in bf16
        t = med(lambda: ops.reparam_fwd(mu_r, mu_i, s2, None, 1, 2, inplace=True))
        out["reparam_fwd@2^20x2048(10B/out bf16, s2 bf16)"] = round(10 * n / t / 1e9, 1)
        t = med(lambda: ops.reparam_bwd(mu_r, mu_i, s2, None, 1, 2, out_dtype=torch.bfloat16))
        out["reparam_bwd@2^20x2048(8B/out bf16, s2 bf16)"] = round(8 * n / t / 1e9, 1)
        del mu_r, mu_i, s2
        # SURVEY 8(d)'s definition of the target: float32 operands, 20 B per output forward / 16 backward
        mu_r = torch.zeros(n, dtype=torch.float32, device=dev)
        mu_i = torch.zeros(n, dtype=torch.float32, device=dev)
        s2 = torch.full((n,), 0.5, dtype=torch.float32, device=dev)
        t = med(lambda: ops.reparam_fwd(mu_r, mu_i, s2, None, 1, 2, inplace=True))
        out["reparam_fwd@2^20x2048(20B/out fp32)"] = round(20 * n / t / 1e9, 1)
        t = med(lambda: ops.reparam_bwd(mu_r, mu_i, s2, None, 1, 2, out_dtype=torch.float32))
        out["reparam_bwd@2^20x2048(16B/out fp32)"] = round(16 * n / t / 1e9, 1)
        del mu_r, mu_i, s2
        m = 16384 * 16384
        wr = torch.randn(m, device=dev) * 0.01
        wi = torch.randn(m, device=dev) * 0.01
        ls2 = torch.empty(m, device=dev).uniform_(-12, 4)
        t = med(lambda: ops.kl_fwd("cplx_vd", wr, wi, ls2))
        out["kl_fwd@16384^2(12B/elt)"] = round(12 * m / t / 1e9, 1)
        t = med(lambda: ops.kl_fwd_bwd("cplx_vd", wr, wi, ls2))
        out["kl_fwd_bwd@16384^2(24B/elt)"] = round(24 * m / t / 1e9, 1)
    except Exception as e:  # pragma: no cover - out of memory on a shared box
        out["error"] = str(e)[:100]
    return out


def conv_point(dev, batch=256, dtype=torch.bfloat16):
    """BASELINE configs[2] beside the headline (rank 0, N = 1, outside the timed region): CplxConv2d(64, 64, 3) on
    256 x 256 bf16 images + CplxBatchNorm2d, forward + backward, channels-last input, `batch` images per step;
    images/s over 10 steps and the three convolution kernels' share of the dense bf16 MFMA peak (HIP events around
    the C-ABI calls: algorithmic 8 B Co Ho Wo Ci 9 flop per launch)."""
    try:
        from cplxmodule_amd import Cplx, nn, conv as cv
        timer = KernelTimer()
        timer.wrap(cv, "cl_conv", lambda *a, **k: "dgrad" if k.get("dgrad") else "fwd")
        timer.wrap(cv, "cl_wgrad", lambda *a, **k: "wgrad")
        # (round 6: the weight-gradient launch that is also the batch-norm layer's backward apply: conv.cl_wgrad_bn)
        timer.wrap(cv, "cl_wgrad_bn", lambda *a, **k: "wgrad")
        torch.manual_seed(0)
        layer, bn = nn.CplxConv2d(64, 64, 3).to(dev), nn.CplxBatchNorm2d(64).to(dev)
        mk = lambda: (torch.randn(batch, 64, 256, 256, device=dev).to(dtype)  # noqa: E731
                      .contiguous(memory_format=torch.channels_last).requires_grad_(True))
        x = Cplx(mk(), mk())

        def step():
            layer.zero_grad(set_to_none=True); bn.zero_grad(set_to_none=True)
            x.real.grad = x.imag.grad = None
            y = bn(layer(x))
            torch.autograd.backward((y.real, y.imag), (y.real.detach(), y.imag.detach()))
        for _ in range(2):
            step()
        timer.enabled = True
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 5
        flop = 8.0 * batch * 64 * 254 * 254 * 64 * 9
        name = "bf16" if dtype == torch.bfloat16 else "fp32"
        out = {"workload": f"CplxConv2d(64,64,3)@256x256 + CplxBatchNorm2d, {name}, batch {batch}, fwd+bwd, channels-last",
               "images_per_s": round(batch / dt, 1), "ms_per_step": round(dt * 1e3, 3), "flop_per_launch": flop}
        if dtype != torch.bfloat16:
            # the 1e-5 mode: three convolutions' flop over the whole step (batch-norm passes included), against the
            # float32-MFMA peak and -- when the half split products ran (conv.py: _x2_conv*) -- against their bound
            from cplxmodule_amd import get_fp32_mode
            out["fp32_mode"] = get_fp32_mode()
            out["tflops_whole_step"] = round(3 * flop / dt / 1e12, 1)
            out["frac_of_fp32_mfma_peak_whole_step"] = round(3 * flop / dt / 1e12 / FP32_PEAK_TFLOPS, 4)
            if _split_kind(out["fp32_mode"]) == "x2":
                out["split_arithmetic"] = "x2"
                out["frac_of_split_bound_whole_step"] = round(3 * flop / dt / 1e12 / SPLIT_BOUND_TFLOPS["x2"], 4)
            return out
        for k in ("fwd", "dgrad", "wgrad"):
            ms = timer.mean_ms(k)
            out[f"{k}_ms"] = round(ms, 4) if ms else None
            out[f"{k}_frac_of_mfma_peak"] = round(flop / (ms * 1e-3) / 1e12 / BF16_PEAK_TFLOPS, 4) if ms else None
        # the forward launch also forms the batch-norm layer's statistics in its epilogue (one pass over y less in the layer;
        # its fraction is still the convolution's flop over the whole launch): CPLXAMD_CONV_BN_MOMENTS=0 for the A/B
        out["bn_moments_in_conv_epilogue"] = bool(cv._MOMENTS and cv._MOMENTS_WANTED)
        # ... and the weight-gradient launch also forms, stores and sums the batch-norm layer's input gradient (the layer's
        # backward apply pass is not launched; `wgrad_ms` includes that work): CPLXAMD_BN_FOLD=0 for the A/B
        out["bn_backward_apply_in_wgrad"] = bool(cv._BN_FOLD)
        return out
    except Exception as e:  # pragma: no cover
        return {"error": str(e)[:200]}


SPLIT_BOUND_TFLOPS = {"x3": BF16_PEAK_TFLOPS / 6.0, "x2": BF16_PEAK_TFLOPS / 3.0}   # piece products per float32 product


def _split_kind(mode):
    from cplxmodule_amd import x3
    return x3.AUTO_KIND if mode == "auto" else (mode if mode in ("x2", "x3") else None)


def fp32_points(dev):
    """The float32 mode -- the one the 1e-5 parity bar is stated in -- at BASELINE's FULL sizes: configs[3] at batch 2^20
    (about 180 GB of float32 planes and 16-bit pieces: only on a GPU with that much free) and configs[2] at batch 256
    channels-last.  Linear layers since round 6: split operands on the 16-bit matrix pipe (cplxmodule_amd/x3.py) -- default
    'x2' = two IEEE-half pieces per operand, three piece products per float32 product (bound 2500 / 3 = 833 TFLOP/s, 2^-22
    norm-wise), `*_x3` = three bf16 pieces, six products (bound 417 TFLOP/s, 2^-24); `*_exact` = the float32-MFMA kernels
    (157.3 TFLOP/s peak) they replaced, same process, for the ratio.  The 3 x 3 convolutions take the half pieces too
    (`x2` only; `conv_cfg3_fp32` vs `_exact`).  Rank 0, N = 1, outside the timed region."""
    out = {"split_bound_tflops": {k: round(v, 1) for k, v in SPLIT_BOUND_TFLOPS.items()}, "fp32_mfma_peak_tflops": FP32_PEAK_TFLOPS}
    try:
        from cplxmodule_amd import fp32_mode
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(dev)
        for tag, mode in (("cfg4_lrt_fp32", "auto"), ("cfg4_lrt_fp32_x3", "x3"), ("cfg4_lrt_fp32_exact", "exact")):
            if free >= 220 << 30:
                with fp32_mode(mode):
                    out[tag] = cfg4_point(dev, dtype=torch.float32, steps=2)
            else:
                out[tag] = {"skipped": f"{free >> 30} GiB free, the float32 step at batch 2^20 wants ~180"}
            torch.cuda.empty_cache()
        for tag, mode in (("conv_cfg3_fp32", "auto"), ("conv_cfg3_fp32_exact", "exact")):
            free, _ = torch.cuda.mem_get_info(dev)
            if free >= 140 << 30:
                with fp32_mode(mode):
                    out[tag] = conv_point(dev, dtype=torch.float32)
            else:
                out[tag] = {"skipped": f"{free >> 30} GiB free"}
            torch.cuda.empty_cache()
        for a, variants in (("cfg4_lrt_fp32", ("", "_x3")), ("conv_cfg3_fp32", ("",))):
            e = out.get(a + "_exact", {})
            for v in variants:
                q = out.get(a + v, {})
                if "ms_per_step" in q and "ms_per_step" in e:
                    q["speedup_over_fp32_mfma_kernels"] = round(e["ms_per_step"] / q["ms_per_step"], 3)
    except Exception as e:  # pragma: no cover
        out["error"] = str(e)[:200]
    return out


def dp_projection(dev):
    """COMPUTE SIDE ONLY -- NOT A SCALING MEASUREMENT.  What one GPU needs for the per-rank share
    of a STRONG-scaling run: the step of configs[1] (+VD) and configs[3] at per-rank batch B / N, N in {1, 2, 4, 8}, on this
    one GPU, eager, with the gradient exchange's host path switched on where a process group exists (world-of-one RCCL
    collectives, bench.py --force-collectives) -- otherwise plain.  The weight-side work (KL, operand preparation, weight
    gradient epilogues, the bucket exchange) does not shrink with N; `ideal_over_this` = (time at N = 1) / (N x time at
    N): the ceiling the compute side puts on strong-scaling efficiency before any link is involved."""
    out = {"note": "compute side only, one GPU, per-rank batch B/N -- not a scaling measurement"}
    try:
        from cplxmodule_amd import Cplx, dp
        from cplxmodule_amd.nn import relevance as rel
        klw = torch.tensor(KLW, device=dev)
        own_group = False
        if not dp.is_initialized():
            # a world-of-one RCCL group for the duration of the sweep, so that the bucket all-reduces are really issued
            # (RCCL prints a banner to stdout when the communicator is created: keep this process's one JSON line clean)
            sys.stdout.flush()
            saved = os.dup(1)
            os.dup2(2, 1)
            try:
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", "29591")
                dp.init_process_group("nccl", device=dev, rank=0, world_size=1)
                own_group = True
                warm = torch.zeros(8, device=dev)
                dist.all_reduce(warm)
                torch.cuda.synchronize()
            except Exception as e:  # pragma: no cover
                out["process_group_error"] = str(e)[:120]
            finally:
                sys.stdout.flush()
                import ctypes
                ctypes.CDLL(None).fflush(None)         # (the banner sits in the C library's stdout buffer)
                os.dup2(saved, 1)
                os.close(saved)
        forced, dp.FORCE_COLLECTIVES = dp.FORCE_COLLECTIVES, dp.is_initialized()
        exchanging = dp._exchanging()
        out["gradient_exchange"] = "RCCL world of one, forced collectives" if exchanging else "none (no process group)"
        for name, feat, full in (("cfg2_vd(4096->4096, global batch 8192)", 4096, 8192),
                                 ("cfg4(2048->2048, global batch 2^20)", 2048, 1 << 20)):
            torch.manual_seed(0)
            layer = rel.CplxLinearVD(feat, feat).to(dev)
            model = dp.DataParallel(layer)
            rows = {}
            for n in (1, 2, 4, 8):
                B = full // n
                x = Cplx(torch.randn(B, feat, device=dev, dtype=torch.bfloat16).requires_grad_(True),
                         torch.randn(B, feat, device=dev, dtype=torch.bfloat16).requires_grad_(True))

                def step():
                    model.zero_grad()
                    x.real.grad = x.imag.grad = None
                    y = model(x)
                    kl = sum(rel.penalties(layer))
                    torch.autograd.backward((y.real, y.imag, kl), (y.real.detach() * 2, y.imag.detach() * 2, klw))
                    model.sync_gradients()
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                k = 3 if full > 8192 else 20
                t0 = time.perf_counter()
                for _ in range(k):
                    step()
                torch.cuda.synchronize()
                rows[n] = (time.perf_counter() - t0) / k * 1e3
                del x
            model.remove()
            out[name] = {f"N={n}": {"per_rank_batch": full // n, "ms_per_step": round(t, 4),
                                     "ideal_over_this": round(rows[1] / (n * t), 4)} for n, t in rows.items()}
            del layer, model
            torch.cuda.empty_cache()
        dp.FORCE_COLLECTIVES = forced
        if own_group:
            dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        out["error"] = str(e)[:200]
    return out


def expected_weak_8(ms_n1, B):
    """What the WEAK-scaling run at N = 8 (8192 rows per GPU, this step on every rank) should print, from this run's
    N = 1 step time and the exchange at link rate -- a projection to hold the driver's SCALE record against, not a
    measurement.  Exchange: one flat float32 bucket set of 3 x 4096^2 + 2 x 4096 gradients = 201 MB per rank
    (log_sigma2, weight.imag, weight.real, biases), mean all-reduce over xGMI (7 links x ~153 GB/s per GPU):
    ring = 2 (7/8) S over ONE link, direct reduce-scatter + all-gather = 2 S / 8 per link over all seven.  The
    weight-gradient buckets are announced before the input-gradient GEMMs (~1.0 ms of launches: dX complex + its
    variance part), which is the window the collective can hide in."""
    S = (3 * IN_F * OUT_F + 2 * OUT_F) * 4.0
    link = 153e9
    ring_ms, direct_ms = 2 * (7 / 8) * S / link * 1e3, 2 * S / 8 / link * 1e3
    window_ms = 1.0
    out = {"per_gpu_batch": B, "bucket_bytes": int(S), "ring_allreduce_ms": round(ring_ms, 3),
           "direct_rs_ag_ms": round(direct_ms, 3), "overlap_window_ms": window_ms, "n1_ms_per_step": round(ms_n1, 4)}
    for name, ex in (("ring", ring_ms), ("direct", direct_ms)):
        for ov, hidden in (("overlapped", min(ex, window_ms)), ("unoverlapped", 0.0)):
            t = ms_n1 + ex - hidden
            out[f"{name}_{ov}"] = {"ms_per_step": round(t, 4), "samples_per_s": round(8 * B / (t * 1e-3), 1),
                                   "efficiency_vs_8x_n1": round(ms_n1 / t, 4)}
    return out


def headline_check(B, dev):
    """bench.py --check: tests/headline_check.py on this workload (graph replay), untimed; errors are reported, not raised."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from headline_check import check_headline_step
        res = check_headline_step(B=B, F=IN_F, graph=True, dev=str(dev))
        return {"passed": True, "against": "float64 numpy + numpy Philox statement (tests/headline_check.py)",
                "max_err_over_max_ref": {k: float(f"{v[0]:.3e}") for k, v in res.items()},
                "asserted": {k: v[1] for k, v in res.items()}}
    except AssertionError as e:
        return {"passed": False, "error": str(e)[:300]}
    except Exception as e:  # pragma: no cover
        return {"passed": None, "error": f"{type(e).__name__}: {str(e)[:300]}"}


DUMP_SAMPLE = 1 << 20


def dump_outputs(out_dir, named):
    """bench.py --dump-outputs: `named` = {name: tensor} of one step, written as float32 <out_dir>/<name>.npy; a tensor
    of more than DUMP_SAMPLE elements is stored as the values at DUMP_SAMPLE flat positions drawn without replacement
    by numpy's default_rng(0) (sorted), the same positions for every tensor of that size and in every run."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    picks = {}
    for name, t in named.items():
        if t is None:
            raise RuntimeError(f"bench.py --dump-outputs: the step produced no {name}")
        a = t.detach()
        n = a.numel()
        if n > DUMP_SAMPLE:
            if n not in picks:
                idx = np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))
                picks[n] = torch.from_numpy(idx).to(a.device)
            a = a.reshape(-1)[picks[n]]
        np.save(os.path.join(out_dir, name + ".npy"), a.float().cpu().numpy())


# The reference itself (PyTorch CPU path of ivannz/cplxmodule) cannot travel to the GPU box; its numbers are the ones taken
# in the build container (BASELINE.md section 2, rows 2 / 2' / 2'' / 4): context beside `cpu_baseline`, never a target.
REFERENCE_CPU = {
    "hardware": "8-core Intel Xeon 2.1 GHz, torch 2.10 CPU kernels (MKL / oneDNN), fp32, measured in the build container",
    "source": "BASELINE.md section 2",
    "cfg2_linear_4m(cplx.linear_naive, B=8192, 4096->4096, fwd+bwd)": {"ms_per_step": 6199, "samples_per_s": 1322},
    "cfg2_linear_3m(cplx.linear_3m)": {"ms_per_step": 3966, "samples_per_s": 2065},
    "cfg2_linear_cat(cplx.linear_cat)": {"ms_per_step": 4703, "samples_per_s": 1742},
    "cfg4_lrt(CplxLinearVD 2048->2048 + exact KL, batch 2^14)": {"ms_per_step": 8723, "samples_per_s": 1878},
}


def gemm_launch_table(spans_mean, B, I, O):
    """{launch: ms}, {launch: fraction of the bf16 MFMA peak} for the GEMM launches a KernelTimer saw (complex 8 B I O flop,
    real 2 B I O; the LRT input gradient with its fused elementwise term is counted with the GEMM's flop only)."""
    launches = {k: round(v, 4) for k, v in sorted(spans_mean.items()) if k[1:5] == "gemm" and v}
    if "cgemm_NT" in launches:
        launches.pop("cgemm_NT_fused_dx", None)      # fallback path: the wrapper timed GEMM + accumulate pass
    cf, rf = 8.0 * B * I * O, 2.0 * B * I * O
    frac = {k: round((cf if k[0] == "c" else rf) / (v * 1e-3) / 1e12 / BF16_PEAK_TFLOPS, 4) for k, v in launches.items()}
    return launches, frac


def cfg4_point(dev, log2_batch=20, timer=None, dtype=torch.bfloat16, batch=None, steps=3):
    """BASELINE configs[3] (rank 0, N = 1, outside the timed region): CplxLinearVD(2048, 2048), bf16 activations, batch
    2^20, LRT forward + fused KL + full backward, loss = sum |y|^2 + 1e-3 KL; ms per step over 3 steps; then one more
    step with HIP events around every GEMM launch (K = 2048: half the K depth of the headline layer)."""
    try:
        from cplxmodule_amd import Cplx
        from cplxmodule_amd.nn import relevance as rel
        torch.manual_seed(0)
        B, F = (1 << log2_batch) if batch is None else batch, 2048
        layer = rel.CplxLinearVD(F, F).to(dev)
        with torch.no_grad():
            layer.log_sigma2.uniform_(-12, 4)
        x = Cplx(torch.randn(B, F, device=dev, dtype=dtype).requires_grad_(True),
                 torch.randn(B, F, device=dev, dtype=dtype).requires_grad_(True))
        klw = torch.tensor(KLW, device=dev)

        def step():
            layer.zero_grad(set_to_none=True)
            x.real.grad = x.imag.grad = None
            y = layer(x)
            kl = sum(rel.penalties(layer))
            gr, gi = y.real.detach() * 2, y.imag.detach() * 2
            torch.autograd.backward((y.real, y.imag, kl), (gr, gi, klw))
        for _ in range(2 if dtype == torch.bfloat16 else 1):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        flop = 3 * (8 + 2) * float(B) * F * F
        bf = dtype == torch.bfloat16
        out = {"workload": f"CplxLinearVD(2048,2048), {'bf16' if bf else 'fp32'}, batch "
                           f"{('2^%d' % log2_batch) if batch is None else batch}, LRT fwd + KL + full bwd",
               "ms_per_step": round(dt * 1e3, 2), "samples_per_s": round(B / dt, 1),
               "tflops_whole_step": round(flop / dt / 1e12, 1),
               ("frac_of_mfma_peak_whole_step" if bf else "frac_of_fp32_mfma_peak_whole_step"):
                   round(flop / dt / 1e12 / (BF16_PEAK_TFLOPS if bf else FP32_PEAK_TFLOPS), 4)}
        if not bf:
            from cplxmodule_amd import get_fp32_mode
            out["fp32_mode"] = get_fp32_mode()
            kind = _split_kind(out["fp32_mode"])
            if kind:                             # (a fraction of the float32-MFMA peak above 1 is possible and means nothing)
                out["split_arithmetic"] = kind
                out["frac_of_split_bound_whole_step"] = round(flop / dt / 1e12 / SPLIT_BOUND_TFLOPS[kind], 4)
        if timer is not None:
            keep, timer.spans, timer.enabled = timer.spans, {}, True
            step()
            torch.cuda.synchronize()
            timer.enabled = False
            means = {k: timer.mean_ms(k) for k in timer.spans}
            timer.spans = keep
            out["launch_ms"], out["launch_frac"] = gemm_launch_table(means, B, F, F)
            out["launch_ms_source"] = "one eager step, HIP events around the C-ABI calls (weight gradients: split-K launch + slab reduce)"
        return out
    except Exception as e:  # pragma: no cover
        return {"error": str(e)[:200]}


def cfg5_point(dev, batch=256, width=8, steps=100):
    """BASELINE configs[4] (rank 0, N = 1, outside the timed region): the Deep-Complex-Net style model of
    examples/train_sparsify.py -- 6 x (CplxConv2d + CplxBatchNorm2d + split ReLU) + CplxLinearARD head, float32 -- on
    synthetic complex MNIST, one train step = forward + cross-entropy + KL + backward + fused Adam, replayed as ONE
    hipGraph per step (a launch-bound model: ~130 kernels of a few microseconds)."""
    import importlib.util
    from cplxmodule_amd.nn import relevance as rel
    from cplxmodule_amd.nn.relevance.noise import noise
    from cplxmodule_amd.utils.graphs import GraphedStep
    old_mode = noise.mode
    try:
        here = os.path.dirname(os.path.abspath(__file__))
        spec = importlib.util.spec_from_file_location("train_sparsify", os.path.join(here, "examples", "train_sparsify.py"))
        ts = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ts)
        torch.manual_seed(0)
        net = ts.Net(rel.CplxLinearARD, width).to(dev)
        x, y = ts.synthetic_complex_mnist(batch, dev, seed=100)
        noise.set_mode("philox-device")
        opt = torch.optim.Adam(net.parameters(), lr=2e-3, capturable=True, fused=True)
        net.train()

        def step():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(net(x), y)
            kl = sum(rel.penalties(net), torch.zeros((), device=dev))
            (loss + 2e-3 * kl).backward()
            opt.step()
            return loss.detach(), kl.detach()

        g = GraphedStep(step, modules=[net], warmup=5)
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            g.replay()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        return {"workload": f"6 x (CplxConv2d + CplxBatchNorm2d + ReLU) + CplxLinearARD, width {width}, complex MNIST 28x28, "
                            f"batch {batch}, float32, fwd + loss + KL + bwd + fused Adam, one hipGraph replay per step",
                "ms_per_step": round(dt * 1e3, 4), "images_per_s": round(batch / dt, 1),
                "loss": round(float(g.outputs[0]), 4)}
    except Exception as e:  # pragma: no cover
        return {"error": str(e)[:200]}
    finally:
        noise.set_mode(old_mode)


def cfg2_point(dev):
    """BASELINE configs[1] as written (rank 0, N = 1, outside the timed region): plain CplxLinear(4096, 4096), bf16,
    batch 8192, forward + backward with the 4-GEMM kernel (`cplx.linear`, one fused 4M launch per pass) and with
    Gauss's 3-GEMM form (`cplx.linear_3m(..., true_3m=True)`; the plain `cplx.linear_3m` call is routed to the 4M kernel
    for bf16 and is timed as "3m"): ms per step and samples/s of each, fraction of the MFMA peak on the flop each
    algorithm must execute (8 / 6 B I O per pass, 3 passes)."""
    try:
        from cplxmodule_amd import Cplx, cplx, nn
        torch.manual_seed(0)
        layer = nn.CplxLinear(IN_F, OUT_F).to(dev)
        x = Cplx(torch.randn(BATCH, IN_F, device=dev, dtype=torch.bfloat16).requires_grad_(True),
                 torch.randn(BATCH, IN_F, device=dev, dtype=torch.bfloat16).requires_grad_(True))
        out = {"workload": "CplxLinear(4096,4096), bf16, batch 8192, fwd+bwd (dX, dW, db)"}
        true_3m = lambda x_, w_, b_: cplx.linear_3m(x_, w_, b_, true_3m=True)  # noqa: E731
        # "3m" = cplx.linear_3m as a user gets it (bf16: routed to the 4M kernel, priced on ITS 8 B I O flop);
        # "3m_true" = the three real MFMA GEMMs + combine (CPLXAMD_TRUE_3M=1), priced on 6 B I O
        for name, fn, mul in (("4m", cplx.linear, 8.0), ("3m", cplx.linear_3m, 8.0), ("3m_true", true_3m, 6.0)):
            def step():
                layer.zero_grad(set_to_none=True)
                x.real.grad = x.imag.grad = None
                y = fn(x, layer.weight, layer.bias)
                torch.autograd.backward((y.real, y.imag), (y.real.detach(), y.imag.detach()))
            for _ in range(8):                     # (the first steps after an idle moment run a few per cent slow)
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 20
            flop = 3 * mul * BATCH * IN_F * OUT_F
            out[name] = {"ms_per_step": round(dt * 1e3, 4), "samples_per_s": round(BATCH / dt, 1),
                         "frac_of_mfma_peak": round(flop / dt / 1e12 / BF16_PEAK_TFLOPS, 4)}
        return out
    except Exception as e:  # pragma: no cover
        return {"error": str(e)[:200]}


def _layout_key(prefix):
    def key(ar, *a, **k):
        if ar.dtype != torch.bfloat16:
            return None
        sa, sb = (a[1], a[4]) if prefix == "cgemm" else (a[0], a[2])
        return f"{prefix}_{'N' if sa[1] == 1 else 'T'}{'N' if sb[1] == 1 else 'T'}"
    return key


def full_headline_figures(timer, graphed, grouped, B):
    """bench.py --full: `roofline` and `hbm_kernels_GBps` of the headline step, from the HIP events `timer` took in the
    eager steps after the timed region (or around the timed launches with --graph off) and, with N = 1, from replays of
    the step's HBM kernels."""
    launches, launch_frac = gemm_launch_table({k: timer.mean_ms(k) for k in timer.spans}, B, IN_F, OUT_F)
    cg = [v for k, v in launches.items() if k.startswith("cgemm")]
    gemm_ms = sum(cg) / len(cg) if cg else None
    traffic, traffic_per = gemm_traffic() if B == BATCH else (None, None)
    flops = 8.0 * B * IN_F * OUT_F          # algorithmic flop of ONE 4M complex GEMM launch
    achieved = flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms else None
    nw = IN_F * OUT_F

    # the step's three HBM kernels: the calls the step made, re-issued ten times in a graph of their own (see replay_ms)
    def replayed(key):
        if grouped:                     # N > 1: other ranks are past this point; nothing extra beside their teardown
            return timer.mean_ms(key)
        try:
            return timer.replay_ms(key)
        except Exception as e:  # pragma: no cover - an auxiliary number must not take the line down
            sys.stderr.write(f"bench.py: replay of {key} failed ({type(e).__name__}: {str(e)[:160]}); event spans instead\n")
            return timer.mean_ms(key)

    pk, rp_f, rp_b = (replayed(k) for k in ("prep_kl", "reparam_fwd", "reparam_bwd"))
    nout = B * OUT_F
    return {
        "roofline": {"bound": "mfma", "kernel": "gemm_bf16_w4_kernel<CPLX> (4M complex GEMM, one wave per SIMD: fwd NN, dgrad NT + fused LRT term, wgrad TT + fused KL accumulate = 3 launches/step)",
                     "achieved": round(achieved, 1) if achieved else None, "peak": BF16_PEAK_TFLOPS,
                     "unit": "TFLOP/s", "frac": round(achieved / BF16_PEAK_TFLOPS, 4) if achieved else None,
                     "traffic": traffic, "traffic_per_launch": traffic_per, "flop_per_launch": flops,
                     "avg_launch_ms": round(gemm_ms, 4) if gemm_ms else None,
                     # every GEMM launch of the step: forward NN, input gradient NT (with the LRT term 2 x ga fused into
                     # its epilogue: counted with the GEMM's 8 B I O flop only), weight gradient TT; complex (8 B I O
                     # flop) and the real variance GEMMs (2 B I O flop)
                     "launch_ms": launches, "launch_frac": launch_frac,
                     # the headline is a graph replay, inside which HIP events cannot be recorded
                     "launch_ms_source": ("ten eager steps right after the timed region (same process, same kernels)"
                                          if graphed else "the timed steps"),
                     "traffic_source": "profiles/ PMC file of these kernels and shapes (bench.py: gemm_traffic), not this run"},
        "hbm_kernels_GBps": {
            # in-step: operand prep + KL sum + KL gradients in one pass (12 B read, 6 + 12 B written)
            "prep_kl_fused(30B/elt)": round(30 * nw / (pk * 1e-3) / 1e9, 1) if pk else None,
            "reparam_fwd(10B/out bf16, s2 bf16)": round(10 * nout / (rp_f * 1e-3) / 1e9, 1) if rp_f else None,
            "reparam_bwd(8B/out bf16, s2 bf16)": round(8 * nout / (rp_b * 1e-3) / 1e9, 1) if rp_b else None,
            "in_step_source": ("HIP events around the Python calls of ten eager steps (spans include allocation and launch gaps)"
                               if grouped else "the step's own calls, ten per hipGraph replay (bench.py: KernelTimer.replay_ms)"),
            "peak": HBM_PEAK_GBS},
    }


def main():
    args = parse()
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_launch(args)                      # does not return
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if args.share_device:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    grouped = world > 1 or args.force_collectives
    # RCCL prints a version banner to STDOUT when a communicator is created; this process owes its caller exactly one
    # JSON line there, so stdout points at stderr until the communicator exists (end of the warm-up)
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    if grouped:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29577")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        # RCCL's kernels must run NEXT TO the input-gradient GEMMs they are meant to overlap: a normal-priority stream can
        # share the compute stream's hardware queue and then runs in queue order (profiles/r03_dp_timeline.txt)
        os.environ.setdefault("TORCH_NCCL_HIGH_PRIORITY", "1")
        if args.rccl_channels > 0:
            os.environ["NCCL_MAX_NCHANNELS"] = str(args.rccl_channels)      # explicit flag wins (dp.init_process_group: max_channels)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    from cplxmodule_amd import Cplx, dp, ops
    from cplxmodule_amd.nn import relevance as rel
    from cplxmodule_amd.nn.relevance import noise
    dp.FORCE_COLLECTIVES = bool(args.force_collectives)

    timer = KernelTimer()
    if args.full:                              # (the per-launch figures of `roofline` / `hbm_kernels_GBps`)
        timer.wrap(ops, "cgemm", _layout_key("cgemm"))       # forward NN, input gradient NT, weight gradient TT
        timer.wrap(ops, "rgemm", _layout_key("rgemm"))
        # the LRT input gradient: G conj(W) + 2 x ga in the epilogue of the persistent (N,T) kernel (one launch); when the
        # kernel declines the shape the call runs cgemm (timed above as cgemm_NT) + the accumulate pass instead
        timer.wrap(ops, "_cplx_lrt_dx", lambda g2r, *a, **k: "cgemm_NT_fused_dx" if g2r.dtype == torch.bfloat16 else None)
        timer.wrap(ops, "prep_kl", lambda *a, **k: "prep_kl" if a[4] else None)
        timer.wrap(ops, "reparam_fwd", lambda *a, **k: "reparam_fwd")
        timer.wrap(ops, "reparam_bwd", lambda *a, **k: "reparam_bwd")

    torch.manual_seed(0)                       # identical init on every rank (then broadcast)
    layer = rel.CplxLinearVD(IN_F, OUT_F).to(dev)
    with torch.no_grad():                      # mixed relevance so both Ei branches are exercised
        layer.log_sigma2.uniform_(-12, 4)
    # gloo (functional tests of the N > 1 path on one GPU) cannot be captured -- its collectives synchronise on the host --
    # so with --graph on the COMPUTE of a step is the graph and the exchange runs behind each replay; every bucket is then
    # reduced in sync_gradients() (overlap=False: the hooks' bookkeeping does not run during a replay)
    split_exchange = grouped and args.backend != "nccl" and args.graph == "on"
    model = dp.DataParallel(layer, overlap=not split_exchange)
    noise.manual_seed(1234 + rank)
    torch.manual_seed(1 + rank)                # per-rank synthetic shard
    B = args.batch
    x = Cplx(torch.randn(B, IN_F, device=dev).bfloat16().requires_grad_(True),
             torch.randn(B, IN_F, device=dev).bfloat16().requires_grad_(True))
    klw = torch.tensor(KLW, device=dev)
    layer.train()

    def compute():
        model.zero_grad()
        x.real.grad = x.imag.grad = None
        y = model(x)
        kl = sum(rel.penalties(layer, reduction="sum"))
        gy_r, gy_i = y.real.detach() * 2, y.imag.detach() * 2      # d(sum |y|^2)/dy
        torch.autograd.backward((y.real, y.imag, kl), (gy_r, gy_i, klw))
        return kl, y.real.detach(), y.imag.detach()          # (the output planes: for --dump-outputs)

    def exchange(out):
        kl, y_r, y_i = out
        model.sync_gradients()
        return (dp.all_reduce_scalar_mean(kl) if grouped else kl), y_r, y_i

    def step():
        return exchange(compute())

    graphed, mode = None, "eager"
    if split_exchange:
        from cplxmodule_amd.utils.graphs import GraphedStep
        noise.set_mode("philox-device")
        inner = GraphedStep(compute, modules=[layer], warmup=max(args.warmup, 3))

        class _ReplayThenExchange:          # same interface as GraphedStep for the timed loop below
            @staticmethod
            def replay():
                model.hook.reset()          # (the buckets' bookkeeping of the previous step; .grad stays the bucket views)
                return exchange(inner.replay())
        graphed, mode = _ReplayThenExchange, "hipGraph replay of the compute + eager gloo exchange"
        graphed.replay()
        torch.cuda.synchronize()
    elif args.graph == "on" and (not grouped or args.backend == "nccl"):
        # W eager warm-up steps on the capture stream, then ONE capture; the timed steps replay it.  (HIP events cannot be
        # recorded inside a replayed graph on ROCm -- "External events are disallowed" -- so the per-launch GEMM times of
        # `roofline` are taken with HIP events around the same launches in ten eager steps right after the timed region.)
        from cplxmodule_amd.utils.graphs import GraphedStep
        noise.set_mode("philox-device")            # Philox position in device memory: fresh noise per replay
        try:
            graphed = GraphedStep(step, modules=[layer], warmup=max(args.warmup, 3))   # (>= 3: communicators, allocator, KL fusion)
            # the W untimed warm-up steps of the contract, as the steps that are timed: replays (the eager steps above exist
            # for the capture; the first replay uploads the graph, and the first three run 5-9 % slow -- clocks and caches
            # after the capture pause -- which with K = 20 was 1.3 % of the reported mean: `step_ms.first_three`)
            for _ in range(max(args.warmup, 1)):
                graphed.replay()
            torch.cuda.synchronize()
            mode = "hipGraph replay"
        except Exception as e:  # pragma: no cover - capture refused: measure the eager path
            sys.stderr.write(f"bench.py: hipGraph capture failed ({type(e).__name__}: {str(e)[:200]}); eager launches\n")
            graphed = None
            noise.set_mode("philox")
    if graphed is None:
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    if grouped:
        dist.barrier()
    torch.cuda.synchronize()
    sys.stdout.flush()
    import ctypes
    ctypes.CDLL(None).fflush(None)             # (the banner sits in the C library's stdout buffer)
    os.dup2(saved_stdout, 1)
    os.close(saved_stdout)
    timer.enabled = args.full and graphed is None
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        out = graphed.replay() if graphed is not None else step()
        marks[i + 1].record()
    torch.cuda.synchronize()
    if grouped:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    timer.enabled = False
    kl = out[0]
    if args.dump_outputs and rank == 0:
        named = {"y_real": out[1], "y_imag": out[2], "x_grad_real": x.real.grad, "x_grad_imag": x.imag.grad}
        named.update(("grad_" + n.replace(".", "_"), p.grad) for n, p in layer.named_parameters())
        named["kl"] = kl
        dump_outputs(args.dump_outputs, named)
    if args.full and graphed is not None:
        timer.enabled = True       # the same launches, eager, HIP events around each: ten steps
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        timer.enabled = False
    if grouped:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt)

    if rank == 0:
        ms = elapsed / args.steps * 1e3
        value = world * B * args.steps / elapsed
        in_order = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
        per = sorted(in_order)
        line = {
            "metric": "Cplx-samples/sec fwd+bwd (CplxLinear-4096 + VD)",
            "value": round(value, 1), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms, 4),
            "step_ms": {"min": round(per[0], 4), "median": round(per[len(per) // 2], 4), "max": round(per[-1], 4),
                        "first_three": [round(v, 4) for v in in_order[:3]]},
            "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "CplxLinearVD 4096->4096, bf16 activations / fp32 master weights, "
                                   f"batch {B} per GPU, LRT fwd + KL + full bwd (BASELINE configs[1] + VD)",
                       "global_batch": world * B, "parallelism": f"dp{world}",
                       "kl_weight": KLW, "noise": "in-kernel Philox4x32-7", "launch": mode,
                       "warmup_detail": (f"{max(args.warmup, 3)} eager steps (capture prerequisites) + {max(args.warmup, 1)} untimed replays"
                                         if graphed is not None else f"{args.warmup} untimed eager steps")},
        }
        if args.full:
            line.update(full_headline_figures(timer, graphed is not None, grouped, B))
        line["kl"] = round(float(kl.detach()), 3)
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["hbm_kernels_GBps"].update(hbm_points(dev))
            line["cfg2_linear"] = cfg2_point(dev)
            line["conv_cfg3"] = conv_point(dev)
            line["cfg4_lrt"] = cfg4_point(dev, timer=timer)
            line["cfg5_train_step"] = cfg5_point(dev)
            line["fp32_full_size"] = fp32_points(dev)
            line["dp_projection"] = dp_projection(dev)
            line["dp_projection"]["expected_weak_8"] = expected_weak_8(ms, B)
            # a figure above what a copy reaches on this chip (6.3 TB/s, MI355X_MICROARCH.md) was not served by HBM: an
            # in-step kernel whose operands the preceding GEMM left in the 256-MiB Infinity Cache.  Mark, do not boast.
            hk = line["hbm_kernels_GBps"]
            hk["cache_assisted"] = {k: True for k, v in list(hk.items())
                                    if isinstance(v, (int, float)) and k != "peak" and v > HBM_COPY_GBS}
            hk["cache_assisted_rule"] = f"> {HBM_COPY_GBS:.0f} GB/s = above the achievable HBM copy rate: fed from the Infinity Cache"
            line["cpu_baseline"] = cpu_baseline(512)
            line["reference_cpu"] = REFERENCE_CPU
        if world == 1 and args.check:
            line["check"] = headline_check(B, dev)
        print(json.dumps(line), flush=True)
    if grouped:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
