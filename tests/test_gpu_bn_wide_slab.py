"""BN slab combines at every slab width: bn_fwd_train and the SyncBatchNorm
pair bn_sync_local / bn_sync_fwd (one rank) fed a hand-made ``pre_stats``
slab [2, C, S].  All tests @pytest.mark.gpu.

The three combine kernels share one summation (bn.hip, bn_slab_sums) whose
order is a function of S alone:

* S <= 1024: a wave per channel, lane l adds entries l, l+64, ... in order
  (at most ceil(S/64) <= 16 additions), then 6 shuffle additions.
* S  > 1024: 16 waves per channel; wave w owns the contiguous share
  [w*ceil(S/16), (w+1)*ceil(S/16)), sums it the same way (ceil(S/1024)
  additions per lane, 6 shuffle additions), and 16 additions in wave order
  join the shares.

What is held:

* Exact data (every entry a small integer, every partial sum below 2^24, so
  no addition rounds): the sums are the float64 sums.  With M = 4 rows the
  division is exact as well, so save_mean and the running mean are
  ``torch.equal`` to the float64 values cast to fp32; save_invstd, scale /
  shift (seen through y) and the running variance are ``torch.equal`` to
  what the same kernel makes of a one-entry slab that holds the float64
  totals cast to fp32 — the tail is a function of the two sums alone.  The
  float64 value of invstd itself is held to 3 ulp: var is exact, var + eps
  rounds once (half an ulp on invstd), rsqrtf is good to 1 ulp, and the
  result is stored rounded.
* Random data: an entry passes at most ceil(S/64) + 6 additions (S <= 1024)
  or ceil(S/1024) + 6 + 16 (S > 1024), and never more than S - 1, because
  lanes past the end of the slab add exact zeros.  Each addition rounds with
  relative error u = 2^-24 on a partial sum no larger than sum|entries|, so
  |sum - sum64| <= S * u * sum|entries|, the bound asserted.
* Plain and sync paths are bit-identical at every S, on any data.
* S <= 1024 keeps the bits of the kernels before the wide path existed:
  tests/golden/bn_slab_narrow.pt holds their outputs for the seeded inputs
  of ``_golden_inputs``.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MOM, EPS = 0.125, 1e-5     # a dyadic momentum: rm = MOM * mean is exact
M_ROWS = 4
CS = [8, 64]
SS = [1, 63, 64, 1024, 1025, 4608, 5408]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "bn_slab_narrow.pt")

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")


def _gen(tag):
    g = torch.Generator()
    g.manual_seed(0x5EED0000 + tag)
    return g


def _x(C):
    """The activations only feed the apply pass; 4 rows of small values."""
    g = _gen(C)
    return (torch.randint(-2, 3, (M_ROWS, C), generator=g).to(torch.bfloat16)
            .to(DEV))


def _exact_slab(C, S):
    """Integers in [-8, 8] (sums), [0, 16] (squares): |partial| <= 16 * 5408
    < 2^24, every addition exact.  The square totals are lifted so that
    var = sq/M - mean^2 stays positive."""
    g = _gen(1000 * C + S)
    a = torch.randint(-8, 9, (C, S), generator=g).double()
    b = torch.randint(0, 17, (C, S), generator=g).double()
    b[:, 0] += (a.sum(1) ** 2 / M_ROWS).ceil().clamp(max=2.0 ** 22) + 1
    assert b.sum(1).max().item() < 2 ** 24 and a.abs().sum(1).max() < 2 ** 24
    return torch.stack([a, b])


def _random_slab(C, S, tag=7):
    g = _gen(1000 * C + S + tag * 100000)
    a = torch.randn(C, S, generator=g, dtype=torch.float64) * 3.0 + 1.0
    b = torch.randn(C, S, generator=g, dtype=torch.float64) ** 2 * 40.0 + 30.0
    return torch.stack([a, b]).float().double()     # fp32-representable


def _golden_inputs(C, S):
    return _random_slab(C, S, tag=11)


def _plain(x, slab64):
    C = x.shape[1]
    g = torch.linspace(0.5, 1.5, C, device=DEV)
    b = torch.linspace(-1.0, 1.0, C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y, sm, si, mask = ext.bn_fwd_train(x, g, b, rm, rv, MOM, EPS, True, None,
                                       slab64.float().to(DEV))
    return y, sm, si, mask, rm, rv


def _sync(x, slab64):
    C = x.shape[1]
    g = torch.linspace(0.5, 1.5, C, device=DEV)
    b = torch.linspace(-1.0, 1.0, C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    row = ext.bn_sync_local(x, slab64.float().to(DEV))
    o = ext.bn_sync_fwd(x, row[None], g, b, rm, rv, MOM, EPS, True)
    return row, (o[0], o[1], o[2], o[3], rm, rv)


CASES = [(C, S) for C in CS for S in SS]
IDS = [f"C{C}-S{S}" for C, S in CASES]


@pytest.mark.parametrize("C,S", CASES, ids=IDS)
def test_exact_sums_equal_the_float64_reduction(C, S):
    x = _x(C)
    slab = _exact_slab(C, S)
    tot = slab.sum(2)                                   # float64 [2, C]
    y, sm, si, mask, rm, rv = _plain(x, slab)
    mean64 = tot[0] / M_ROWS
    assert torch.equal(sm.cpu(), mean64.float())
    assert torch.equal(rm.cpu(), (MOM * mean64.float()))
    var64 = tot[1] / M_ROWS - mean64 ** 2
    assert var64.min().item() > 0
    inv64 = (var64 + EPS).rsqrt()
    assert ((si.cpu().double() - inv64).abs() <= 3 * 2 * U * inv64).all()
    # the tail is a function of the totals alone: a one-entry slab of them
    one = _plain(x, tot[:, :, None])
    for got, want, name in zip((y, sm, si, mask, rm, rv), one,
                               ("y", "mean", "invstd", "mask", "rm", "rv")):
        assert torch.equal(got, want), name
    row, sync = _sync(x, slab)
    assert torch.equal(row[:2 * C].cpu(), tot.reshape(-1).float())
    assert row[2 * C:].tolist() == [0, M_ROWS]
    for got, want, name in zip(sync, (y, sm, si, mask, rm, rv),
                               ("y", "mean", "invstd", "mask", "rm", "rv")):
        assert torch.equal(got, want), "sync " + name


@pytest.mark.parametrize("C,S", CASES, ids=IDS)
def test_random_sums_within_the_chain_bound_and_paths_agree(C, S):
    x = _x(C)
    slab = _random_slab(C, S)
    tot, mag = slab.sum(2), slab.abs().sum(2)
    row, sync = _sync(x, slab)
    got = row[:2 * C].cpu().double().reshape(2, C)
    err = (got - tot).abs()
    print(f"C={C} S={S}: max err/(S u mag) = "
          f"{(err / (S * U * mag)).max().item():.3e}")
    assert (err <= S * U * mag).all()
    plain = _plain(x, slab)
    for got_t, want, name in zip(sync, plain,
                                 ("y", "mean", "invstd", "mask", "rm", "rv")):
        assert torch.equal(got_t, want), name
    # the plain path's sums are the row's: mean * 4 is an exact scaling
    assert torch.equal(plain[1] * M_ROWS, row[:C])


def test_narrow_slabs_keep_their_bits():
    gold = torch.load(GOLDEN)
    n = 0
    for C in CS:
        for S in [s for s in SS if s <= 1024]:
            x = _x(C)
            slab = _golden_inputs(C, S)
            row, _ = _sync(x, slab)
            _, sm, si, _, rm, rv = _plain(x, slab)
            want = gold[f"C{C}-S{S}"]
            for got, name in ((row, "row"), (sm, "mean"), (si, "invstd"),
                              (rm, "rm"), (rv, "rv")):
                assert torch.equal(got.cpu(), want[name]), (C, S, name)
            n += 1
    assert n == len(gold) == 8
