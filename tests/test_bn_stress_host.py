"""The ill-conditioned batch-norm cases (tests/bn_stress_cases.py) on the host: the numpy oracle against the float64
results of the reference recorded in tests/golden/bn_stress.npz (so that the oracle can judge the kernels where the
reference does not exist), and the cap on the reference's own float32 error that keeps the GPU assertions meaningful."""
import os

import numpy as np
import pytest

import bn_stress_cases as sc
from oracle import cplx_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_stress.npz")
CAP = 1e-2          # 4 e_ref above this: max(1e-5, 4 e_ref) would pass a kernel that is wrong in the third digit


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN)


def test_the_grid_is_the_one_the_fixture_was_recorded_for(fixture):
    """Nothing dropped silently: the conditions every tier has to hold, every case in the fixture, every route a case."""
    C = sc.Cond
    mild, hard, tiny, bf = (set(sc.TIERS[k]) for k in ("mild", "hard", "tiny", "bf16"))
    for s in sc.SCALES:
        for rho in ("r0", "r9"):
            assert {C(0, rho, s), C(10, rho, s)} <= mild and {C(100, rho, s), C(1000, rho, s)} <= hard
        assert {C(0, "r999", s), C(10, "r999", s), C(100, "r999", s)} <= hard
        assert any(c.kind == "im0" and c.scale == s for c in mild)
    assert {C(0, "lin", 0.3), C(10, "lin", 0.3), C(100, "lin", 0.1), C(0, "lin", 1e-3), C(0, "lin", 1e-6)} <= mild | hard
    assert {c.kind for c in tiny} == {"r0", "r9", "r999", "lin", "im0", "const"}
    assert {c.ratio for c in bf} == {0, 2, 8, 32} and {"r0", "r9", "r999", "lin", "im0", "const"} == {c.kind for c in bf}
    assert any(c.kind == "const" for c in mild)
    counts = {int(np.prod(sc.BY_NAME[n].shape)) // sc.BY_NAME[n].shape[1] for n in sc.COUNT_CASES}
    assert counts == {1, 2, 3}
    for case in sc.CASES:
        for mode, qs in (("train", sc.QUANTITIES), ("eval", sc.EVAL_QUANTITIES)):
            for q in qs:
                assert f"{case.name}/{mode}/e_ref/{q}" in fixture.files, (case.name, mode, q)
    # shapes: [B, F], small planes, large planes, S % 4 != 0, channels-last rows, F not a multiple of 8 / of 64
    f32 = [sc.BY_NAME[n] for n in sc.F32_CASES]
    S = lambda c: int(np.prod(c.shape[2:]))  # noqa: E731
    assert any(len(c.shape) == 2 for c in f32) and any(1 < S(c) < 1024 for c in f32) and any(S(c) >= 1024 for c in f32)
    assert any(S(c) >= 1024 and S(c) % 4 for c in f32) and any(1 < S(c) < 1024 and S(c) % 4 for c in f32)
    assert any(c.cl and c.shape[1] % 8 == 0 and c.shape[0] * S(c) >= 4096 for c in f32)
    assert any(c.cl and c.shape[1] % 8 for c in f32) and any(c.shape[1] % 64 for c in f32)


@pytest.mark.parametrize("name", sc.F32_CASES)
def test_reference_float32_error_is_finite_and_under_the_cap(fixture, name):
    for mode, qs in (("train", sc.QUANTITIES), ("eval", sc.EVAL_QUANTITIES)):
        for q in qs:
            e = float(fixture[f"{name}/{mode}/e_ref/{q}"])
            assert np.isfinite(e) and 4 * e <= CAP, (name, mode, q, e)


@pytest.mark.parametrize("name", sc.STORED_CASES)
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_oracle_reproduces_the_float64_reference(fixture, name, mode):
    """1e-10 norm-wise per feature, at mean / std up to 1000, correlation 0.999, xi = c xr, scales 1e-6 ... 1e6."""
    d = sc.build(name)
    floor = sc.floors(d)
    got = sc.oracle_results(orc, d, np.float64, training=mode == "train")
    for q in (sc.QUANTITIES if mode == "train" else sc.EVAL_QUANTITIES):
        ref = fixture[f"{name}/{mode}/f64/{q}"]
        e = sc.rel_per_feature(sc.as_feature_rows(q, got[q]), sc.as_feature_rows(q, ref), floor.get(q))
        f = int(np.argmax(e))
        assert e[f] <= 1e-10, (name, mode, q, e[f], tuple(d["conds"][f]))


def test_inputs_are_what_the_table_says():
    """The generator of the inputs itself: realised mean / std and correlation, exactness of xi = c xr, bf16 values."""
    d = sc.build("cols_hard")
    for f, c in enumerate(d["conds"]):
        u, v = d["xr"][:, f].astype(np.float64), d["xi"][:, f].astype(np.float64)
        if c.kind in ("r0", "r9", "r999"):
            assert abs(u.mean() / u.std() - c.ratio) < 0.15 + 0.1 * c.ratio          # (the sample std of 1024 draws: +- 2 %)
            rho = np.corrcoef(u, v)[0, 1]
            assert abs(rho - {"r0": 0.0, "r9": 0.9, "r999": 0.999}[c.kind]) < (0.1 if c.kind == "r0" else 0.02 if c.kind == "r9" else 3e-4)
            assert 1.2 * c.scale < u.std() < 1.8 * c.scale
        if c.kind == "lin":
            assert np.array_equal(d["xi"][:, f], np.float32(sc.LIN_C) * d["xr"][:, f])
        if c.kind == "im0":
            assert not d["xi"][:, f].any()
    b = sc.build("cols_bf16")
    for k in ("xr", "xi", "gr", "gi"):
        assert np.array_equal(b[k], sc.bf16_round(b[k]))
    try:
        import torch
    except ImportError:
        return
    a = np.random.RandomState(0).randn(4096).astype(np.float32) * 37
    assert np.array_equal(sc.bf16_round(a), torch.from_numpy(a).bfloat16().float().numpy())
