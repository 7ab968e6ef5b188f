"""The elementwise sweep without a GPU (tests/elementwise_cases.py): the case tables cannot thin themselves out, the bounds
are attainable by the formulas of csrc/cplxfn.hip as written (a float32 numpy restatement), the part-overflow guard
tells the fixed product forms from the old ones, the edge tables reach vector bodies and tails, and the util.hip group's
entry points refuse a misaligned pointer before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import elementwise_cases as ec

DTYPES = (torch.float32, torch.bfloat16)


def test_wrap_lengths_come_from_the_source_constants():
    assert ec.GRID_CAP == 2048 and set(ec.BLOCK.values()) == {256}
    assert ec.wrap_length("cplxfn", torch.float32) == 2097152 and ec.wrap_length("cplxfn", torch.bfloat16) == 4194304
    assert ec.wrap_length("layout", torch.bfloat16) == ec.wrap_length("util", torch.bfloat16) == 2097152
    assert max(max(ec.sizes(g, d)) for g in ec.BLOCK for d in DTYPES) == 4194304 + 11       # the largest tensor of the sweep
    for g in ec.BLOCK:
        for d in DTYPES:
            assert ec.sizes(g, d)[:len(ec.SMALL_SIZES)] == ec.SMALL_SIZES and ec.PERIOD % ec.vec(g, d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fn", ec.FUNCTIONS)
def test_every_family_keeps_its_points(fn, dtype):
    """from the reference alone: the masks drop no more than the case module says they must"""
    for name in ec.families(fn):
        r = ec.reference(fn, name, dtype)
        assert np.isfinite(r["f"].real).all() and np.isfinite(r["f"].imag).all() or fn == "log", (fn, name)
        keep = ec._in_mask(r["f"]).mean()
        assert keep >= ec.keep_min(fn, name), (fn, name, keep)
        if name == "part_overflow" and fn in ec.PRODUCT_FORM:
            assert ec.has_part(r["f"]) >= ec.part_keep_min(dtype), (fn, ec.has_part(r["f"]))
            assert keep < 0.01                    # the family is past the modulus mask: that is what it is for
        bk = (ec._in_mask(r["scale"]) & np.isfinite(r["d"])).mean()
        if name != "part_overflow":
            assert bk >= ec.keep_min(fn, name, backward=True), (fn, name, bk)


def test_keep_floors_below_the_default_are_few():
    assert len(ec.KEEP_MIN_FWD) == 6 and len(ec.KEEP_MIN_BWD) == 7
    assert all(f == "seam88" or f == "part_overflow" for _, f in list(ec.KEEP_MIN_FWD) + list(ec.KEEP_MIN_BWD))


@pytest.mark.parametrize("fn", ec.FUNCTIONS)
def test_closed_form_backward_agrees_with_complex128_autograd(fn):
    """reference()['d'] is conj(f') g with a closed-form f'; complex128 autograd through the cancellation-free spelling of
    tests/test_gpu_cplx_fn.py gives the same to 1e-7 |f'| |g| (2^-7 u; the pole neighbourhood of tan / tanh costs the most)"""
    for name in ec.families(fn):
        if name == "part_overflow":
            continue
        r = ec.reference(fn, name)
        ag = ec.autograd_backward(fn, name)
        m = ec._in_mask(r["scale"]) & np.isfinite(ag)
        if m.any():
            assert (np.abs(ag - r["d"])[m] <= 1e-7 * r["scale"][m]).all(), (fn, name)


@pytest.mark.parametrize("fn", ec.FUNCTIONS)
def test_restated_formulas_stay_inside_the_bounds(fn):
    """float32, every family but part_overflow, forward (modulus-wise and per part) and backward"""
    for name in ec.families(fn):
        if name == "part_overflow":
            continue
        zr, zi, gr, gi = (t.numpy() for t in ec.points(fn, name))
        r = ec.reference(fn, name)
        worst, part, keep, _ = ec.forward_ratios(fn, torch.float32, *ec.emulate(fn, zr, zi), r["f"])
        assert worst <= 1 and (part is None or part <= 1), (fn, name, worst, part)
        # the restatement with correctly rounded functions needs about half the bound (the issue: 5.1 u modulus-wise, 7.2 u
        # per part of 16 u): the rest is the device functions' 1-2 ulp
        assert worst <= 0.5 and (part is None or part <= 0.5), (fn, name, worst, part)
        bw, _, small = ec.backward_ratios(torch.float32, *ec.emulate_backward(fn, zr, zi, gr, gi), r)
        assert bw <= 0.5 and small, (fn, name, bw, small)


@pytest.mark.parametrize("fn", ec.PRODUCT_FORM)
def test_part_overflow_guard_tells_the_fixed_forms_from_the_old(fn):
    zr, zi, _, _ = (t.numpy() for t in ec.points(fn, "part_overflow"))
    f = ec.reference(fn, "part_overflow")["f"]
    _, part, _, pkeep = ec.forward_ratios(fn, torch.float32, *ec.emulate(fn, zr, zi, fixed=True), f)
    assert part <= 0.5 and pkeep > 0.2, (part, pkeep)
    _, old, _, _ = ec.forward_ratios(fn, torch.float32, *ec.emulate(fn, zr, zi, fixed=False), f)
    assert old == np.inf                              # e^x * cos y: inf or NaN where the part is representable


def test_special_table_has_a_decided_reference_and_the_restatement_meets_it():
    table = ec.special_table()
    ref = ec.special_reference(table)
    assert len(table) >= 40
    for (fn, a, b), (rr, ri) in zip(table, ref):
        assert not np.isnan(rr) and not np.isnan(ri), (fn, a, b)
        gr, gi = ec.emulate(fn, np.array([a], np.float32), np.array([b], np.float32))
        assert ec.same_special(float(gr[0]), rr) and ec.same_special(float(gi[0]), ri), (fn, a, b, gr, gi, rr, ri)


def test_edge_tables_put_special_values_into_bodies_and_tails():
    assert len(ec.EDGE_Z) % 2 == 1 and len(ec.EDGE_W) % 2 == 1 and len(ec.EDGE_TAU) % 2 == 1 and len(ec.EDGE_MASK) % 2 == 1
    for n in ec.SMALL_SIZES + (ec.wrap_length("layout", torch.float32) + 7,):
        if n < 5:
            continue
        zr, zi, tau, wr, wi, mask = ec.edge_planes(n)
        sp = ec.is_special(zr, zi)
        body = 4 * (n // 4)
        quads = sp[:body].reshape(-1, 4)
        assert quads.any(axis=1).all(), n                       # every aligned quad holds one
        for v in (8,):                                          # (and every aligned group of 8: bf16 in cplxfn.hip)
            assert sp[:v * (n // v)].reshape(-1, v).any(axis=1).all()
        if n % 4:
            assert sp[body:].any(), n                           # and so does the tail
        wsp = ~np.isfinite(wr) | ~np.isfinite(wi) | (np.abs(wr) >= 1e20) | (np.hypot(wr, wi) < 1e-29)
        msp = ~np.isfinite(mask) | (mask == 0)
        assert (tau < 0)[:body].any()
        assert wsp[:body].reshape(-1, 4).any(axis=1).all() and msp[:body].reshape(-1, 4).any(axis=1).all(), n
    # what the table is there for: all of these occur
    zr, zi = ec.EDGE_Z[:, 0], ec.EDGE_Z[:, 1]
    m = np.hypot(zr.astype(np.float64), zi.astype(np.float64))
    assert np.signbit(zr[(zr == 0)]).any() and (np.abs(zr[zr != 0]) < 1e-38).any()
    assert ((m > 0) & (m < 1e-5)).any() and ((m >= 1e-5) & (m < 2e-5)).any()
    assert (np.abs(m - 0.5) <= 2 * 2.0 ** -24).sum() >= 4 and (m == 0.5).any() and (m > 0.5)[np.abs(m - 0.5) < 1e-6].any()
    assert np.isinf(zr).any() and np.isinf(zi).any() and np.isnan(zr).any() and (np.abs(zr) == np.float32(1e20)).any()
    assert (ec.EDGE_TAU < 0).any()


def test_float32_chains_are_the_documented_operations():
    """mul / div chain against complex128 on tame values (it is an implementation of the product, not of something else),
    and the overflow / underflow quotients the edge table locks in"""
    rs = np.random.RandomState(0)
    a, b, c, d = (rs.randn(4096).astype(np.float32) for _ in range(4))
    z, w = a.astype(np.float64) + 1j * b, c.astype(np.float64) + 1j * d
    for div, ref in ((False, z * w), (True, z / w)):
        re, im = ec.mul_chain(a, b, c, d, div)
        assert (np.abs((re + 1j * im) - ref) <= 8 * ec.U * np.abs(z) * (np.abs(w) if not div else 1 / np.abs(w))).all()
    one = np.float32(1.0)
    re, im = ec.mul_chain(one, one, np.float32(1e20), one, div=True)          # c^2 overflows: p = c / inf = 0
    assert re == 0 and im == 0
    re, im = ec.mul_chain(one, one, np.float32(1e-30), np.float32(1e-30), div=True)   # c^2 + d^2 underflows to 0: c / 0
    assert np.isnan(re) or np.isinf(re)
    x = np.array([-1.0, -0.0, 0.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
    assert np.array_equal(ec.split_relu_chain(x), torch.relu(torch.from_numpy(x)).numpy(), equal_nan=True)


def test_pool_cases_hold_ties_and_enough_configurations():
    zr, zi = ec.pool_planes()
    m = ec.pool_modulus(zr, zi)
    assert m.dtype == np.float32 and (m == 5).sum() >= 8            # 3+4i, 4+3i, 5, 5i, ...
    assert len({(a, b) for a, b in zip(zr[m == 5], zi[m == 5])}) >= 4
    assert np.isnan(ec.pool_planes(nan=True)[0]).sum() == 5
    cfgs = ec.pool_configs()
    assert 150 <= len(cfgs) <= 4 * 4 * 2 * 3 * 2 and len(set(cfgs)) == len(cfgs)
    ties = 0
    for cfg in cfgs:
        k, s, p, d, ceil = cfg
        _, idx = torch.nn.functional.max_pool2d(torch.from_numpy(m), k, s, p, d, ceil, return_indices=True)
        mx = torch.nn.functional.max_pool2d(torch.from_numpy(m), k, s, p, d, ceil)
        # a window with a tie: its maximum occurs at another position of the plane that the window also covers -- counted
        # loosely by the maxima that are 5 (several Gaussian integers share that modulus)
        ties += int((mx == 5).sum())
        yr, yi, idx2, gr, gi, dzr, dzi = ec.pool_reference(zr, zi, cfg)
        assert torch.equal(idx, idx2) and float(dzr.sum()) == float(gr.sum()) and float(dzi.sum()) == float(gi.sum())
    assert ties > 1000


# ---- C: the alignment contract of the util.hip group ------------------------------------------------------------------
def _util_calls(lib, F32, BF16):
    """name -> (number of plane pointers, optional positions, call(pointers, n, dtype))"""
    return {
        "cplxamd_cplx_abs_fwd": (3, (), lambda p, n, dt: lib.cplxamd_cplx_abs_fwd(*p, n, dt, None)),
        "cplxamd_cplx_abs_bwd": (5, (), lambda p, n, dt: lib.cplxamd_cplx_abs_bwd(*p, n, dt, None)),
        "cplxamd_mask_mul": (5, (1, 4), lambda p, n, dt: lib.cplxamd_mask_mul(*p, n, dt, F32 + BF16 - dt, None)),
        "cplxamd_abs2": (3, (1,), lambda p, n, dt: lib.cplxamd_abs2(*p, n, dt, F32 + BF16 - dt, None)),
        "cplxamd_modulus": (3, (), lambda p, n, dt: lib.cplxamd_modulus(*p, n, None)),
        "cplxamd_exp": (2, (), lambda p, n, dt: lib.cplxamd_exp(*p, n, dt, None)),
        "cplxamd_cast": (2, (), lambda p, n, dt: lib.cplxamd_cast(*p, n, dt, F32 + BF16 - dt, None)),
        "cplxamd_lrt_dx_accum": (5, (1, 3), lambda p, n, dt: lib.cplxamd_lrt_dx_accum(*p, n, dt, F32 + BF16 - dt, None)),
    }


def test_util_entry_points_refuse_misaligned_pointers_without_a_gpu():
    """never dereferenced: every call below is refused, or has nothing to do, before a launch"""
    from cplxmodule_amd import _lib
    lib = _lib.load()
    good, bad4, bad8 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1008)
    for name, (k, optional, call) in _util_calls(lib, _lib.F32, _lib.BF16).items():
        for dt in (_lib.F32, _lib.BF16):
            assert call([good] * k, 0, dt) == 0, name                       # aligned, nothing to do
            assert call([good] * k, -1, dt) == -1, name
            for i in range(k):
                for bad in (bad4, bad8):                                    # (0x1008: element-aligned for either dtype)
                    p = [good] * k
                    p[i] = bad
                    assert call(p, 16, dt) == -2, (name, i)
                    assert call(p, 0, dt) == -2, (name, i)                  # checked before the n == 0 return, as layout.hip
                p = [good] * k
                p[i] = None
                if i not in optional:
                    assert call(p, 16, dt) == -1, (name, i)                 # a missing plane is EINVAL, before alignment
            if optional:                                                    # absent optional planes: NULL is not misaligned
                p = [None if i in optional else good for i in range(k)]
                assert call(p, 0, dt) == 0, name
                p[0] = bad4
                assert call(p, 16, dt) == -2, name
        if name not in ("cplxamd_modulus",):
            assert call([good] * k, 0, 7) == -1, name                       # unknown dtype


def test_header_states_the_alignment_contract():
    import os
    import re
    src = open(os.path.join(ec.ROOT, "include", "cplxamd.h")).read()
    m = re.search(r"elementwise / layout helpers used by the layers(.*?)\*/", src, flags=re.S)
    assert m and "16-byte aligned" in m.group(1) and "CPLXAMD_EALIGN" in m.group(1)
    for name in ("abs2", "_modulus", "_cplx_abs_fwd", "_cplx_abs_bwd", "_mask_mul", "_exp", "_cast", "_lrt_dx_accum"):
        assert name in m.group(1), name
