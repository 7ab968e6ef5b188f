"""The masked layers' route on compacted operands, host side (no GPU): the granule padding, the flag plumbing and the
report on CPU-resident modules, and the GEMM dispatch at compacted shapes."""
import itertools

import numpy as np
import pytest
import torch

from cplxmodule_amd import compact
from cplxmodule_amd.nn import masked


@pytest.mark.parametrize("total", [1, 63, 64, 65, 130, 257, 1030])
def test_pad_live_properties(total):
    rs = np.random.RandomState(total)
    lives = [[], [0], [total - 1], list(range(total)), list(range(0, total, 2)), list(range(max(total - 3, 0), total))]
    lives += [sorted(rs.choice(total, size=rs.randint(1, total + 1), replace=False).tolist()) for _ in range(8)]
    for live in lives:
        out = compact.pad_live(live, total)
        assert out == sorted(out) and len(set(out)) == len(out)                  # ascending, no repeats
        assert set(live) <= set(out)                                              # superset of the live set
        assert all(0 <= i < total for i in out) and len(out) <= total             # never exceeds `total`
        if not live:
            assert out == []                                                      # empty stays empty
        else:
            assert len(out) % 64 == 0 or len(out) == total                        # a multiple of the granule, or everything
            assert len(out) == min(total, -(-len(live) // 64) * 64)
            # the padding is the LOWEST-numbered dead indices
            dead = [i for i in range(total) if i not in set(live)]
            assert sorted(set(out) - set(live)) == dead[:len(out) - len(live)]


def test_pad_live_nearly_full_total_not_a_multiple():
    total = 130                                     # 2 * 64 + 2: a nearly full live set cannot be rounded up past total
    assert compact.pad_live(range(129), total) == list(range(130))
    assert compact.pad_live(range(1, 130), total) == list(range(130))
    assert compact.pad_live(range(128), total) == list(range(128))
    assert compact.pad_live([5], total, granule=4) == [0, 1, 2, 5]
    with pytest.raises(ValueError):
        compact.pad_live([130], total)


def _net():
    return torch.nn.Sequential(masked.CplxLinearMasked(8, 6), masked.LinearMasked(6, 5), masked.CplxConv2dMasked(3, 4, 3),
                               masked.Conv2dMasked(3, 4, 3), masked.CplxConv1dMasked(3, 4, 3), masked.Conv1dMasked(3, 4, 3),
                               masked.CplxConv3dMasked(2, 2, 1), masked.Conv3dMasked(2, 2, 1),
                               masked.CplxBilinearMasked(3, 3, 2), masked.BilinearMasked(3, 3, 2))


def test_compact_flag_sets_and_unsets_and_is_not_state():
    net = _net()
    keys = list(net.state_dict().keys())
    assert not any(m.compact for m in net)
    assert masked.compact_(net) is net
    assert [m.compact for m in net] == [True] * 4 + [False] * 6                   # the other layers ignore the flag
    assert list(net.state_dict().keys()) == keys
    assert all(m.compact_max_live is None for m in net)
    masked.compact_(net, max_live=0.25)
    assert [m.compact_max_live for m in net][:5] == [0.25] * 4 + [None]
    # survives mask_() and load_state_dict
    net[1].mask = torch.ones(5, 6)
    net.load_state_dict(net.state_dict(), strict=False)
    assert net[1].compact and net[1].compact_max_live == 0.25
    assert "compact" not in "".join(net.state_dict().keys())
    masked.compact_(net, enabled=False)
    assert not any(m.compact for m in net)


def test_compaction_report_on_cpu_modules():
    net = _net()
    masked.compact_(net, max_live=1.0)
    rep = masked.compaction(net)
    assert set(rep) == {str(i) for i in range(10)} and all(v is None for v in rep.values())     # no masks yet
    m = torch.ones(6, 8)
    m[1] = 0
    m[4] = 0
    m[:, 5] = 0
    net[0].mask = m
    mc = torch.ones(4, 3, 3, 3)
    mc[:, 1] = 0
    mc[2] = 0
    net[3].mask = mc
    net[4].mask = torch.ones(4, 3, 3)
    net[9].mask = torch.ones(2, 3, 3)
    rep = masked.compaction(net)
    assert rep["0"] == dict(rows=(4, 6, 6), cols=(7, 8, 8), active=False)          # padded to the full size: dense
    assert rep["3"] == dict(rows=(3, 4, 4), cols=(2, 3, 3), active=False)
    assert rep["4"] is None and rep["9"] is None and rep["1"] is None              # no route / no mask
    big = masked.LinearMasked(256, 192)
    mb = torch.zeros(192, 256)
    mb[5:60, 100:130] = 0.5                                                         # soft entries are live
    big.mask = mb
    assert masked.compaction(big)[""] == dict(rows=(55, 64, 192), cols=(30, 64, 256), active=False)   # flag off
    masked.compact_(big)
    assert masked.compaction(big)[""]["active"] is True                            # 64 * 64 / (192 * 256) <= 0.5
    masked.compact_(big, max_live=0.01)
    assert masked.compaction(big)[""]["active"] is False
    with torch.no_grad():
        big.mask[100, 200] = 1.0                                                    # an in-place edit is seen
    assert masked.compaction(big)[""]["rows"] == (56, 64, 192) and masked.compaction(big)[""]["cols"] == (31, 64, 256)
    big.mask = torch.zeros(192, 256)
    assert masked.compaction(big)[""] == dict(rows=(0, 0, 192), cols=(0, 0, 256), active=True)     # nothing left to run
    grouped = masked.Conv2dMasked(128, 128, 1, groups=2)
    grouped.mask = torch.zeros(128, 64, 1, 1)
    masked.compact_(grouped, max_live=1.0)
    assert masked.compaction(grouped)[""]["active"] is False                       # groups > 1 run dense
    dbl = masked.LinearMasked(256, 192).double()
    dbl.mask = mb
    masked.compact_(dbl, max_live=1.0)
    assert masked.compaction(dbl)[""]["active"] is False                           # float64 runs dense


def test_compacted_shapes_stay_on_the_fast_gemm_family():
    """B = 8192, (O', I') in {64, 192, 4032}^2: cplxamd_gemm_plan picks an MFMA kernel kind (non-zero; 0 is the generic
    kernel) for the forward, the input-gradient and the weight-gradient layouts, as it does at 4096^2 -- the granule keeps
    compacted shapes away from the generic kernel."""
    from cplxmodule_amd import _lib
    L = _lib.load()
    BF, F32, B = _lib.BF16, _lib.F32, 8192
    plan = lambda *a: L.cplxamd_gemm_plan(*a, 0, 256)  # noqa: E731

    def kinds(cplx, O, I):
        return (plan(cplx, B, O, I, 0, 0, BF, 0),            # forward  [B, I] x [O, I]^T
                plan(cplx, B, I, O, 0, 1, BF, 1 if cplx else 0),   # input gradient  [B, O] x [O, I]
                plan(cplx, O, I, B, 1, 1, F32, 2))           # weight gradient  [B, O]^T x [B, I]
    for cplx in (1, 0):
        assert all(k > 0 for k in kinds(cplx, 4096, 4096))
        for O, I in itertools.product((64, 192, 4032), repeat=2):
            assert all(k > 0 for k in kinds(cplx, O, I)), (cplx, O, I, kinds(cplx, O, I))
