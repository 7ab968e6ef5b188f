"""nn.init without a GPU: the three torch-RNG initialisers bit for bit against the reference's recorded planes, the two
Trabelsi initialisers (orthogonality, standard deviation, statistics), cplx_polar_factor's host twin of the device
recurrence against the float64 SVD polar factor, the in-place contract, and the argument checks of the cplxamd_init_*
entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cplxmodule_amd import Cplx
from cplxmodule_amd.nn import init

import init_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("cplxamd_init_ws_bytes", "cplxamd_init_moments", "cplxamd_init_ns_poly", "cplxamd_init_scale_store")
# the reference's own smoke and orthogonality cases (tests/test_init.py:29-68)
WEIGHTS = (((500, 1250), torch.float32), ((1250, 500), torch.float32), ((32, 64, 3, 3), torch.float32),
           ((3, 7, 5, 5), torch.float64))


def test_public_names():
    assert set(init.__all__) == {"get_fans", "cplx_kaiming_normal_", "cplx_xavier_normal_", "cplx_kaiming_uniform_",
                                 "cplx_xavier_uniform_", "cplx_trabelsi_standard_", "cplx_trabelsi_independent_",
                                 "cplx_uniform_independent_", "cplx_polar_factor"}
    import cplxmodule_amd.nn
    for name in init.__all__:
        assert callable(getattr(cplxmodule_amd.nn.init, name))


# ---- 1. bit identity with the reference ----------------------------------------------------------------------------------
def test_torch_rng_initialisers_equal_the_reference_bit_for_bit():
    fx = C.fixture()
    assert [str(n) for n in fx["thin_names"]] == list(C.NEW[:3])
    for name in C.NEW[:3]:
        for shape in ((6, 10), (4, 3, 2, 2)):
            for dtype, dn in ((torch.float32, "f32"), (torch.float64, "f64")):
                w = Cplx.empty(*shape, dtype=dtype)
                torch.manual_seed(int(fx["thin_seed"]))
                assert getattr(init, name)(w) is w
                np.testing.assert_array_equal(w.real.numpy(), fx[f"thin_{name}_{C.tag(shape)}_{dn}_re"])
                np.testing.assert_array_equal(w.imag.numpy(), fx[f"thin_{name}_{C.tag(shape)}_{dn}_im"])
    # the non-default arguments reach torch's initialisers as the reference passes them
    a, b = Cplx.empty(6, 10), Cplx.empty(6, 10)
    torch.manual_seed(3)
    init.cplx_kaiming_normal_(a, a=0.5, mode="fan_out", nonlinearity="leaky_relu")
    torch.manual_seed(3)
    for plane in (b.real, b.imag):
        torch.nn.init.kaiming_normal_(plane, a=np.sqrt(1 + 2 * 0.25), mode="fan_out", nonlinearity="leaky_relu")
    assert np.array_equal(C.c128(a), C.c128(b))
    torch.manual_seed(3)
    init.cplx_xavier_uniform_(a, gain=3.0)
    torch.manual_seed(3)
    for plane in (b.real, b.imag):
        torch.nn.init.xavier_uniform_(plane, gain=3.0 / np.sqrt(2))
    assert np.array_equal(C.c128(a), C.c128(b))


# ---- 2. smoke and orthogonality, 3. standard deviation -------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", WEIGHTS, ids=lambda v: C.tag(v) if isinstance(v, tuple) else str(v)[6:])
def test_all_five_run_and_the_orthogonal_one_is_orthogonal(shape, dtype):
    torch.manual_seed(17)
    for name in C.NEW:
        w = Cplx.empty(*shape, dtype=dtype)
        assert getattr(init, name)(w) is w
        assert np.isfinite(C.c128(w)).all() and np.abs(C.c128(w)).max() > 0, name
    for kind in C.KINDS:
        w = Cplx.empty(*shape, dtype=dtype)
        C.check_independent(init.cplx_trabelsi_independent_(w, kind=kind), kind)


def test_kind_in_any_letter_case_and_bf16_storage():
    torch.manual_seed(18)
    for kind in ("Glorot", "XAVIER", "KaiMing", "HE"):
        for shape, dtype in (((3, 7, 5, 5), torch.float64), ((48, 80), torch.float32)):
            C.check_independent(init.cplx_trabelsi_independent_(Cplx.empty(*shape, dtype=dtype), kind=kind), kind)
        a, b = Cplx.empty(8, 12), Cplx.empty(8, 12)
        torch.manual_seed(1)
        init.cplx_trabelsi_standard_(a, kind=kind)
        torch.manual_seed(1)
        init.cplx_trabelsi_standard_(b, kind=kind.lower())
        assert np.array_equal(C.c128(a), C.c128(b))
    for shape in ((48, 80), (8, 6, 3, 3)):
        C.check_independent(init.cplx_trabelsi_independent_(Cplx.empty(*shape, dtype=torch.bfloat16)))


# ---- 4. statistics of the standard initialiser ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("glorot", "he"))
def test_trabelsi_standard_statistics(kind):
    """Five standard errors each, N = 625 000 complex entries with independent N(0, scale^2) parts:
    |w|^2 / scale^2 is chi^2_2 (mean 2, sd 2): the mean of |w|^2 has relative standard error 1 / sqrt N;
    the unit phasor has sd 1 / sqrt 2 per part: its mean has standard error 1 / sqrt(2 N);
    re * im has sd scale^2: standard error scale^2 / sqrt N;
    a plane's sample std has relative standard error 1 / sqrt(2 N)."""
    shape = (500, 1250)
    scale = float(C.fixture()[f"scale_{C.tag(shape)}_{kind}"])
    torch.manual_seed(23)
    w = C.c128(init.cplx_trabelsi_standard_(Cplx.empty(*shape), kind=kind))
    N = w.size
    assert N == 625000
    assert abs((np.abs(w) ** 2).mean() / (2 * scale ** 2) - 1) <= 5 / np.sqrt(N)
    ph = (w / np.abs(w)).mean()
    assert abs(ph.real) <= 5 / np.sqrt(2 * N) and abs(ph.imag) <= 5 / np.sqrt(2 * N)
    assert abs((w.real * w.imag).mean()) <= 5 * scale ** 2 / np.sqrt(N)
    for plane in (w.real, w.imag):
        assert abs(plane.std() / scale - 1) <= 5 / np.sqrt(2 * N)


# ---- 5. the polar factor against the SVD ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("f32", "f64"))
def test_polar_factor_against_the_float64_svd(dtype):
    """max |M - U V^H| <= 64 u (float32) / 128 u (float64).  Host route, observed: float32 at most 6.4 u ((64, 64)),
    float64 at most 13.4 u ((33, 33)) on one host, 10.8 u ((64, 64)) on
    another: the same seeds, another BLAS summation order."""
    for i, shape in enumerate(C.POLAR_SHAPES):
        z = C.gaussian(shape, dtype, 100 + i)
        err = C.polar_error(z, init.cplx_polar_factor(z))
        print(f"polar host {shape} {dtype}: {err:.2f} u")
        assert err <= C.POLAR_BOUND[dtype], shape
    # orthonormal columns (tall) / rows (wide)
    m = C.c128(init.cplx_polar_factor(C.gaussian((130, 67), dtype, 7)))
    assert np.abs(m.conj().T @ m - np.eye(67)).max() <= 32 * C.U[dtype]
    m = C.c128(init.cplx_polar_factor(C.gaussian((21, 25), dtype, 8)))
    assert np.abs(m @ m.conj().T - np.eye(21)).max() <= 32 * C.U[dtype]


def test_polar_factor_of_bf16_and_of_a_strided_input():
    z = C.gaussian((21, 25), torch.bfloat16, 9)
    m = init.cplx_polar_factor(z)
    assert m.dtype == torch.bfloat16 and m.shape == z.shape
    assert np.abs(C.c128(m) - C.svd_polar(z)).max() <= C.U[torch.bfloat16] + 64 * C.U[torch.float32]   # entries are below 1
    base = C.gaussian((25, 21), torch.float64, 10)
    np.testing.assert_array_equal(C.c128(init.cplx_polar_factor(base.t())),
                                  C.c128(init.cplx_polar_factor(Cplx(base.real.t().contiguous(), base.imag.t().contiguous()))))


# ---- 6. contract ---------------------------------------------------------------------------------------------------------
def test_same_seed_same_draw_next_call_another():
    C.check_seeding("cpu")


def test_writes_reach_the_parameters_of_layers():
    C.check_layers("cpu")


def test_non_contiguous_tensors_are_filled_in_place():
    C.check_strided("cpu")


def test_requires_grad_is_kept_and_no_graph_is_recorded():
    C.check_autograd_flags("cpu")


def test_one_dimensional_tensors_and_bad_kinds_are_rejected():
    C.check_rejections("cpu")


def test_polar_factor_raises_on_zero_nonfinite_and_rank_deficient_input():
    C.check_polar_failures("cpu")


def test_a_draw_over_the_step_cap_is_drawn_again(monkeypatch):
    C.check_redraw("cpu", monkeypatch)


# ---- 7. exports ----------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_exported_under_abi_25():
    from cplxmodule_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cplxamd.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert "#define CPLXAMD_ABI_VERSION 25" in src and _lib.ABI_VERSION == 25
    enum = re.search(r"enum\s*\{\s*CPLXAMD_INIT_SCALE_NORM[^}]*\}", src).group(0)
    assert re.findall(r"CPLXAMD_INIT_SCALE_([A-Z]+)\s*=\s*(\d)", enum) == [("NORM", "0"), ("STD", "1"), ("CONST", "2")]
    assert (_lib.INIT_SCALE_NORM, _lib.INIT_SCALE_STD, _lib.INIT_SCALE_CONST) == (0, 1, 2)
    lib = ctypes.CDLL(os.path.join(ROOT, "cplxmodule_amd", "libcplxamd.so"))
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert _lib.load().cplxamd_abi_version() == 25
    assert _lib.load().cplxamd_init_ws_bytes() >= 3 * 8


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from cplxmodule_amd import _lib
    lib = _lib.load()
    ok = ctypes.c_void_p(0x1000)            # never dereferenced: every case below is refused before a launch
    mom = lambda re=ok, im=ok, n=16, dt=_lib.F32, out=ok, ws=ok: lib.cplxamd_init_moments(re, im, n, dt, out, ws, None)  # noqa: E731
    assert mom(re=None) == -1 and mom(im=None) == -1 and mom(out=None) == -1 and mom(ws=None) == -1
    assert mom(n=0) == -1 and mom(n=-5) == -1
    assert mom(dt=_lib.BF16) == -1 and mom(dt=_lib.F16) == -1 and mom(dt=7) == -1 and mom(dt=-1) == -1

    def poly(gr=ok, gi=ok, pr=ok, pi=ok, k=8, dt=_lib.F64, res=ok, ws=ok):
        return lib.cplxamd_init_ns_poly(gr, gi, pr, pi, k, 1.5, -0.5, dt, res, ws, None)
    assert poly(gr=None) == -1 and poly(gi=None) == -1 and poly(pr=None) == -1 and poly(pi=None) == -1
    assert poly(res=None) == -1 and poly(ws=None) == -1 and poly(k=0) == -1 and poly(k=-3) == -1
    assert poly(dt=_lib.BF16) == -1 and poly(dt=9) == -1

    def store(ir=ok, ii=ok, our=ok, oui=ok, rows=5, cols=3, tr=0, mode=_lib.INIT_SCALE_STD, target=1.0, m=ok, idt=_lib.F32,
              odt=_lib.BF16):
        return lib.cplxamd_init_scale_store(ir, ii, our, oui, rows, cols, tr, mode, target, m, None, idt, odt, None)
    assert store(ir=None) == -1 and store(ii=None) == -1 and store(our=None) == -1 and store(oui=None) == -1
    assert store(rows=0) == -1 and store(cols=-1) == -1 and store(rows=2 ** 31) == -1
    assert store(idt=_lib.BF16) == -1 and store(idt=5) == -1 and store(odt=_lib.F16) == -1 and store(odt=4) == -1
    assert store(idt=_lib.F32, odt=_lib.F64) == -1 and store(idt=_lib.F64, odt=_lib.BF16) == -1      # not a parameter's cast
    assert store(mode=3) == -1 and store(mode=-1) == -1 and store(target=float("nan")) == -1
    assert store(m=None) == -1 and store(m=None, mode=_lib.INIT_SCALE_NORM) == -1
    assert store(rows=2 ** 31 - 1, cols=2 ** 31 - 1, tr=1) == -3        # more than 2^31 - 1 tiles
