"""The case tables of the L0 / LASSO / LRT noise sweep (tests/l0_sweep_cases.py) without a GPU: every case reaches the branch
it is named for (column step and trip counts of the forward, plan fields of the per-column backward, body / tail / wrap of
the streaming kernels), the bounds are attainable -- a float32 numpy restatement of the gate in l0.hip's header stays
within a quarter of TOL_Z and TOL_DZ of the float64 oracle on the very data of every GPU case -- and no case has more than
EXCLUDE_CAP of its elements in the clamp band."""
import numpy as np
import pytest

import l0_sweep_cases as lc

BLOCK = 1 << 21


@pytest.fixture(scope="module")
def stream():
    """the uniform stream at (SEED, OFFSET) up to the largest case, once"""
    n = max([lc.A_MAX] + [r * c for r, c, *_ in lc.B_CASES.values()])
    return np.concatenate([lc.uniform_window(e, min(e + BLOCK, n)) for e in range(0, n, BLOCK)])


def _attainable(la, u, what, capped=True):
    """worst float32-restatement error / bound on (z, dz) and the band's share, blockwise"""
    la = np.asarray(la).reshape(-1)
    worst_z = worst_dz = 0.0
    excluded = 0
    for e in range(0, la.size, BLOCK):
        lb = la[e:e + BLOCK]
        ub = None if u is None else np.asarray(u).reshape(-1)[e:e + BLOCK]
        z, dz, pre = lc.gate64(lb, ub)
        z32, dz32, _ = lc.gate32(lb, ub)
        assert np.isfinite(z32).all() and np.isfinite(dz32).all(), what
        out = ~lc.band(pre)
        excluded += int((~out).sum())
        worst_z = max(worst_z, float(np.abs(z32 - z).max()) / lc.TOL_Z)
        if out.any():
            worst_dz = max(worst_dz, float(np.abs(dz32 - dz)[out].max()) / lc.TOL_DZ)
    assert worst_z <= lc.COVERAGE and worst_dz <= lc.COVERAGE, (what, worst_z, worst_dz)
    if capped:
        assert excluded <= lc.EXCLUDE_CAP * la.size, (what, excluded, la.size)
    return worst_z, worst_dz


def test_constants_are_read_from_the_sources():
    assert lc.L8 == 8 * lc.L1 == 8 * lc.GRID_CAP * lc.L0_THREADS and lc.RP_L8 == 8 * lc.GRID_CAP * lc.RP_THREADS
    assert lc.SEED == 2 ** 64 - 1 and lc.OFFSET == 2 ** 40 + 3
    assert lc.TOL_S * 1.2 == pytest.approx(lc.TOL_Z) and lc.TOL_DZ == pytest.approx(1e-5 / 0.66)
    s = np.linspace(0, 1, 100001)
    assert np.abs(1.2 / 0.66 * (1 - 2 * s)).max() <= 1.82 and (1.2 / 0.66 * s * (1 - s)).max() == pytest.approx(lc.DZ_MAX)


def test_windows_equal_the_stream_and_sit_on_every_seam(stream):
    for n in (1, 5, lc.L1 + 9, 2 * lc.L8 + 24):
        ws = lc.windows(n)
        assert ws[0][0] == 0 and ws[-1][1] == n
        for L in (lc.L1, lc.L8):
            for m in range(L, n, L):
                assert any(a < m < b or (a < m and b == n) for a, b in ws), (n, m)
        for a, b in ws:
            assert 0 < b - a <= lc.WINDOW
            np.testing.assert_array_equal(lc.uniform_window(a, b), stream[a:b])
    assert stream.dtype == np.float32 and stream.min() >= lc.U_MIN and stream.max() <= lc.U_MAX
    # the noise windows are those of oracle/philox.py
    from oracle import philox
    np.testing.assert_array_equal(lc.normal_window(5, 1031, False, 7, 3), philox.real_noise(1031, 7, 3)[5:])
    rr, ri = philox.cplx_noise(1031, 7, 3)
    wr, wi = lc.normal_window(3, 1031, True, 7, 3)
    np.testing.assert_array_equal(wr, rr[3:])
    np.testing.assert_array_equal(wi, ri[3:])


def test_elementwise_sizes_reach_body_tail_and_wrap():
    stride = lc.GRID_CAP * lc.L0_THREADS
    for n in lc.A_VECTOR:
        assert n % 8 == 0
    trips = [-(-(n // 8) // stride) for n in lc.A_VECTOR]
    assert trips == [1, 1, 2, 3]                                      # L8 - 8, L8: the last single trip; then 2 and 3
    for n in lc.A_SCALAR:
        assert n % 8 != 0                                             # the forward's scalar form
    assert [-(-n // stride) for n in lc.A_SCALAR] == [1, 2, 2]
    (n,) = lc.A_MIXED
    assert n % 8 == 5 and (n // 8) > stride                           # the backward: wrapped vector body + 5-element tail
    assert {n % 8 for n in lc.A_SMALL} >= {0, 1, 7} and max(lc.A_SMALL) > 8 * lc.L0_THREADS


@pytest.mark.parametrize("name", list(lc.B_CASES))
def test_forward_cases_take_their_column_step(name):
    rows, cols, vec, trips, dc = lc.B_CASES[name]
    assert lc.fwd_walk(rows, cols) == (vec, trips, dc)
    if dc is not None and dc != 0:
        # the wrap `c >= cols` is taken by some thread and not by another
        c0 = (8 * np.arange(min(rows * cols // 8, lc.GRID_CAP * lc.L0_THREADS))) % cols
        assert ((c0 + dc) >= cols).any() and ((c0 + dc) < cols).any()


def test_forward_cases_cover_every_walk():
    walks = [lc.fwd_walk(r, c) for r, c, *_ in lc.B_CASES.values()]
    assert any(v and t >= 3 and dc for v, t, dc in walks) and any(v and t >= 3 and dc == 0 for v, t, dc in walks)
    assert any(not v and t == 2 for v, t, dc in walks)


@pytest.mark.parametrize("name", list(lc.C_CASES))
def test_backward_cases_take_their_plan(name):
    from cplxmodule_amd import _lib
    rows, cols, want = lc.C_CASES[name]
    plan = lc.cols_plan(rows, cols)
    for k, v in want.items():
        assert plan[k] == v, (name, k, plan)
    nbytes = int(_lib.load().cplxamd_l0_gate_bwd_ws_bytes(rows, cols))
    assert nbytes == 4 * cols * plan["chunks"], (name, plan)
    assert not plan["capped"]


def test_backward_cases_cover_every_plan_branch():
    from cplxmodule_amd import _lib
    plans = {k: lc.cols_plan(r, c) for k, (r, c, _) in lc.C_CASES.items()}
    rows = {k: v[0] for k, v in lc.C_CASES.items()}
    for V in (1, 8):
        assert any(p["V"] == V and p["strips"] > 1 and p["last_strip_groups"] < p["TX"] for p in plans.values())
        assert any(p["V"] == V and p["idle"] > 0 for p in plans.values())
        assert any(p["V"] == V and rows[k] == 1 for k, p in plans.items())
    assert any(rows[k] < p["TY"] and rows[k] > 1 for k, p in plans.items())
    assert any(p["chunks"] > 1 and p["last_chunk_rows"] < p["rows_per_chunk"] for p in plans.values())
    assert any(p["strips"] == 3 for p in plans.values())
    cap = lc.cols_plan(*lc.C_CAP)
    assert cap["capped"] and cap["rows_per_chunk"] == 17 and cap["chunks"] == 1000
    assert int(_lib.load().cplxamd_l0_gate_bwd_ws_bytes(*lc.C_CAP)) == 4 * lc.C_CAP[1] * cap["chunks"]
    assert lc.C_CAP[0] * lc.C_CAP[1] <= 35_000_000


def test_bounds_attainable_elementwise(stream):
    la, _, _ = lc.elem_data(lc.A_MAX)                                 # every size is a prefix of this draw
    wz, wd = _attainable(la, stream[:lc.A_MAX], "A train")
    ez, ed = _attainable(la, None, "A eval")
    print(f"\nl0_sweep host A: float32 restatement / bound: train z {wz:.3f} dz {wd:.3f}, eval z {ez:.3f} dz {ed:.3f}")
    for n in lc.A_SIZES:                                              # the cap holds for every prefix that can hold one
        if n >= 2000:
            pre = lc.gate64(la[:n], stream[:n])[2]
            assert lc.band(pre).sum() <= lc.EXCLUDE_CAP * n, n


@pytest.mark.parametrize("name", list(lc.B_CASES) + list(lc.C_CASES) + [f"E{r}x{c}" for r, c in lc.E_SHAPES])
def test_bounds_attainable_per_column(stream, name):
    if name in lc.B_CASES:
        rows, cols = lc.B_CASES[name][:2]
    elif name in lc.C_CASES:
        rows, cols = lc.C_CASES[name][:2]
    else:
        rows, cols = map(int, name[1:].split("x"))
    la = lc.cols_data(rows, cols)[0]
    full = np.broadcast_to(la, (rows, cols)).reshape(-1)
    _attainable(full, stream[:rows * cols], name + " train")
    _attainable(la, None, name + " eval")


@pytest.mark.parametrize("train", [True, False])
def test_edge_tables_hold_what_they_name(train):
    la, u, runs = lc.edge_table(train)
    assert la.shape[1] == 64 and la.dtype == np.float32
    z, dz, pre = lc.gate64(la, u)
    assert np.isfinite(z).all() and np.isfinite(dz).all()
    assert set(np.float32(lc.EDGE_LA)) <= set(la.reshape(-1))
    if train:
        assert (u == lc.U_MIN).any() and (u == lc.U_MAX).any() and u.min() >= lc.U_MIN and u.max() <= 1
        near0, near1 = np.abs(pre) < lc.TOL_Z, np.abs(pre - 1) < lc.TOL_Z     # the +-8 neighbours of pre = 0 and pre = 1
        assert near0.sum() == 7 * 17 and near1.sum() == 7 * 17
        assert np.abs(pre).min() < 1e-6 and np.abs(pre - 1).min() < 1e-6
        assert (pre[near0] < 0).any() and (pre[near0] > 0).any() and (pre[near1] < 1).any() and (pre[near1] > 1).any()
    else:
        assert len(runs) == 2
        flat, p = la.reshape(-1), pre.reshape(-1)
        for a, b in runs:
            assert b - a == 129 and (np.diff(flat[a:b]) > 0).all()
        a, b = runs[0]
        assert p[a] > 0 > p[b - 1] and flat[a + 64] == np.float32(lc.LN11)      # pre crosses 0 inside the run
        a, b = runs[1]
        assert p[a] > 1 > p[b - 1]
    assert (pre < -lc.TOL_Z).any() and (pre > 1 + lc.TOL_Z).any()
    _attainable(la, u, "edge table", capped=False)                    # z everywhere, dz outside the band


def test_lasso_pattern_and_thresholds():
    p = lc.l1_pattern(lc.PERIOD)
    assert (p == 0).any() and np.signbit(p[p == 0]).any() and np.isnan(p).any() and np.isinf(p).any()
    assert ((np.abs(p) > 0) & (np.abs(p) < np.finfo(np.float32).tiny)).any() and (np.abs(p) == np.finfo(np.float32).max).any()
    lo, t, hi = lc.l1_thresholds()
    assert lo < t < hi and np.float32(t) == lc.l1_log(p[lc.F_PIVOT:lc.F_PIVOT + 1])[0]
    w = lc.l1_pattern(lc.L1 + 3)
    m_lo, m_t, m_hi = (lc.l1_ref(w, x) for x in (lo, t, hi))
    pivot = w == p[lc.F_PIVOT]
    assert pivot.sum() > 2 * (w.size // lc.PERIOD)
    assert m_lo[pivot].all() and m_t[pivot].all() and not m_hi[pivot].any()     # the mask flips exactly there
    assert (m_lo == m_t).all() and (m_t != m_hi).sum() == pivot.sum()
    assert not lc.l1_ref(np.float32([np.nan]), -1e30)[0] and lc.l1_ref(np.float32([np.inf, -np.inf]), 80.0).all()
    # |w| + 1e-20f in float32: zeros and subnormals land on log(1e-20f)
    assert (lc.l1_log(np.float32([0.0, -0.0, 1e-40])) == np.float32(np.log(np.float64(np.float32(1e-20))))).all()
    stride = lc.GRID_CAP * lc.L0_THREADS
    assert [-(-n // stride) for n in lc.F_SIZES] == [1, 1, 1, 1, 1, 2]


def test_reparam_cases_reach_body_tail_and_wrap():
    from cplxmodule_amd import _lib
    stride = lc.GRID_CAP * lc.RP_THREADS
    trips = {n: -(-(n >> 3) // stride) for n in lc.G_SIZES}
    assert trips[lc.RP_L8 + 8 + 3] == 2 and (lc.RP_L8 + 8 + 3) % 8 == 3 and trips[2 * lc.RP_L8 + 16] == 3
    assert {n % 8 for n in lc.G_SIZES} >= {0, 1, 3, 7} and trips[2055] == 1
    for n in lc.G_SIZES:
        d = lc.reparam_data(n)
        assert all(v.size == n and v.dtype == np.float32 for v in d.values())
        k = min(4, n)
        np.testing.assert_array_equal(d["s2"][:k], np.float32(lc.G_SPECIAL)[:k])
        if n >= 16:
            v0 = ((n >> 3) - 1) << 3
            np.testing.assert_array_equal(d["s2"][v0:v0 + 4], np.float32(lc.G_SPECIAL))
    s2 = np.float32(lc.G_SPECIAL)
    _, _, gs2, sd = lc.reparam_ref(s2, None, s2, s2 + 1, None, s2 + 1, None)
    assert list(gs2 != 0) == [False, False, True, True] and sd[0] == sd[1] == sd[2]       # passes AT 1e-8, blocked below
    for rows, cols in lc.G_COLS:
        assert rows * cols > lc.RP_L8 and int(_lib.load().cplxamd_lrt_reparam_bwd_cols_ws_bytes(rows, cols)) > 0
