"""GPU tier of global gradient-norm clipping: the multi-tensor square-sum /
finalize / scale kernels and the lazy clip inside fused_sgd.

Shapes are the smallest at which the (tensor, 16384-element chunk) mapping
can go wrong: sizes around the chunk edge, a 70-tensor list (crosses two
32-tensor launch groups, so the partial index must be global) and views of
one flat at element offsets that are not 16-byte aligned.  Every tensor is
carved out of a sentinel-filled flat with one guard element on each side,
so an out-of-range write shows up as a changed guard value.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

CH = 16384
SIZES = [0, 1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 7]
GUARD = -12345.0


def _ext():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    assert ext.MT_CHUNK == CH
    return ext


def _cases():
    """name -> (sizes, lead): tensors packed into one flat after `lead`
    elements, one guard element between neighbours."""
    c = {f"n{n}": ([n], 0) for n in SIZES}
    c["all_sizes"] = (SIZES, 0)
    c["seventy_by_5"] = ([5] * 70, 0)
    for off in (1, 2, 3):
        c[f"offset{off}"] = ([CH + 1, 7, 2 * CH + 7], off)
    return c


CASES = _cases()


def _pack(cpu_tensors, lead):
    """Device views of one sentinel flat at arbitrary element offsets (what
    p.grad is inside a DDP bucket).  Returns (views, flat, guard_mask)."""
    total = lead + sum(t.numel() + 1 for t in cpu_tensors) + 1
    flat = torch.full((total,), GUARD, dtype=torch.float32)
    guard = torch.ones(total, dtype=torch.bool)
    spans, pos = [], lead + 1
    for t in cpu_tensors:
        n = t.numel()
        flat[pos:pos + n] = t
        guard[pos:pos + n] = False
        spans.append((pos, n))
        pos += n + 1
    dflat = flat.to(DEV)
    views = [dflat.narrow(0, s, n) for s, n in spans]
    return views, dflat, guard


def _guards_intact(dflat, guard):
    return bool((dflat.cpu()[guard] == GUARD).all())


def _nchunks(tensors):
    return sum((t.numel() + CH - 1) // CH for t in tensors)


def _int_tensors(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-2, 3, (n,), generator=g).float() for n in sizes]


def _chunk_sqsums(cpu_tensors):
    out = []
    for t in cpu_tensors:
        for c in range((t.numel() + CH - 1) // CH):
            out.append(float(t[c * CH:(c + 1) * CH].double().pow(2).sum()))
    return out


def _finalize(ext, partials, n, max_norm=0.0, found_inf=None, stats=None):
    out = torch.full((2,), -1.0, device=DEV)
    ext.norm_finalize(partials, n, max_norm, found_inf, out, stats)
    return out.cpu()


# ------------------------------------------------------ 1. exact arithmetic ---

@pytest.mark.parametrize("case", list(CASES))
def test_exact_square_sums(case):
    """Values in {-2..2}: every partial and the total are integers far below
    2**24, so fp32/fp64 sums are exact in any order."""
    ext = _ext()
    sizes, lead = CASES[case]
    cpu = _int_tensors(sizes, seed=11)
    views, dflat, guard = _pack(cpu, lead)
    want = _chunk_sqsums(cpu)
    n = len(want)
    assert n == _nchunks(cpu)
    total = int(sum(want))
    assert total < 2 ** 24
    partials = torch.full((n + 3,), GUARD, device=DEV)
    ext.multi_tensor_sqsum(views, partials)
    got = partials.cpu()
    assert got[:n].tolist() == want              # global partial index
    assert bool((got[n:] == GUARD).all())        # nothing written past n
    assert _guards_intact(dflat, guard)          # read-only kernel
    for v, t in zip(views, cpu):
        assert torch.equal(v.cpu(), t)
    assert int(got[:n].double().sum()) == total
    out = _finalize(ext, partials, n)
    # double sqrt is correctly rounded; one rounding to fp32 on top
    assert float(out[0]) == float(np.float32(math.sqrt(total)))
    assert float(out[1]) == 1.0

    # the fused unscale (x4 -> *0.25, exact) gives the same partials
    views4, dflat4, guard4 = _pack([t * 4 for t in cpu], lead)
    fi = torch.zeros(1, device=DEV)
    p2 = torch.full((n + 3,), GUARD, device=DEV)
    ext.multi_tensor_unscale(views4, fi, 0.25, p2)
    assert torch.equal(p2.cpu(), got)
    assert float(fi) == 0.0
    assert _guards_intact(dflat4, guard4)
    for v, t in zip(views4, cpu):
        assert torch.equal(v.cpu(), t)


@pytest.mark.parametrize("sizes,lead,norm", [
    ([CH], 0, 128.0),
    ([1, CH - 1], 1, 128.0),
    ([CH + 1, 3 * CH - 1], 3, 256.0),
    ([4], 2, 2.0),
])
def test_perfect_square_norm(sizes, lead, norm):
    """All-ones tensors totalling 4**k elements: the norm is that integer."""
    ext = _ext()
    cpu = [torch.ones(n) for n in sizes]
    assert sum(sizes) == int(norm) ** 2
    views, _, _ = _pack(cpu, lead)
    n = _nchunks(cpu)
    partials = torch.zeros(n, device=DEV)
    ext.multi_tensor_sqsum(views, partials)
    assert float(_finalize(ext, partials, n)[0]) == norm


def test_partials_too_small_is_an_error():
    ext = _ext()
    views, _, _ = _pack([torch.ones(CH + 1)], 0)     # 2 chunks
    small = torch.zeros(1, device=DEV)
    fi = torch.zeros(1, device=DEV)
    with pytest.raises(RuntimeError, match="partials"):
        ext.multi_tensor_sqsum(views, small)
    with pytest.raises(RuntimeError, match="partials"):
        ext.multi_tensor_unscale(views, fi, 1.0, small)
    with pytest.raises(RuntimeError, match="partials"):
        ext.norm_finalize(small, 2, 0.0, None, torch.zeros(2, device=DEV),
                          None)
    assert bool((views[0].cpu() == 1).all())


# ----------------------------------------------------------- 2. random data ---

@pytest.mark.parametrize("case", ["all_sizes", "seventy_by_5", "offset1",
                                  "offset2", "offset3"])
def test_random_norm_matches_float64(case):
    """<= 64 serial fp32 adds per thread + an 8-level tree over positive
    terms: relative error of the sum <= ~72 * 2**-24 = 4.3e-6, half that on
    the norm; 1e-5 leaves ~4x margin."""
    from ddp_tricks_amd.ops import clip_grad_norm_
    sizes, lead = CASES[case]
    g = torch.Generator().manual_seed(21)
    cpu = [torch.randn(n, generator=g) for n in sizes]
    want = float(torch.linalg.vector_norm(torch.cat(cpu).double()))
    views, dflat, guard = _pack(cpu, lead)
    got = clip_grad_norm_(views, 0.0)            # measure only
    assert got.device == DEV and got.dim() == 0
    assert abs(float(got) - want) <= 1e-5 * want
    assert _guards_intact(dflat, guard)
    # and clipping: same coefficient as the CPU formula, applied in place
    max_norm = 0.5 * want
    got = clip_grad_norm_(views, max_norm)
    assert abs(float(got) - want) <= 1e-5 * want
    coef = float((max_norm / (got.cpu() + 1e-6)).clamp(max=1.0))
    for v, t in zip(views, cpu):
        assert torch.allclose(v.cpu(), t * coef, rtol=1e-6, atol=0)
    assert _guards_intact(dflat, guard)


# ------------------------------------------------- 3. fused equals separate ---

@pytest.mark.parametrize("case", ["all_sizes", "seventy_by_5", "offset1",
                                  "offset3"])
def test_fused_unscale_equals_separate(case):
    ext = _ext()
    sizes, lead = CASES[case]
    g = torch.Generator().manual_seed(31)
    cpu = [torch.randn(n, generator=g) * 1000.0 for n in sizes]
    n = _nchunks(cpu)
    inv = 1.0 / 4096.0 / 3.0                     # not a power of two

    def plain():
        views, dflat, guard = _pack(cpu, lead)
        fi = torch.zeros(1, device=DEV)
        ext.multi_tensor_unscale(views, fi, inv)
        return views, dflat, guard, fi

    def fused():
        views, dflat, guard = _pack(cpu, lead)
        fi = torch.zeros(1, device=DEV)
        partials = torch.full((n,), GUARD, device=DEV)
        ext.multi_tensor_unscale(views, fi, inv, partials)
        return views, dflat, guard, fi, partials

    va, fa, ga, fia = plain()
    vb, fb, gb, fib, pb = fused()
    assert torch.equal(fa, fb)                   # tensors AND guards
    assert _guards_intact(fb, gb)
    assert float(fia) == 0.0 and float(fib) == 0.0
    ps = torch.full((n,), GUARD, device=DEV)
    ext.multi_tensor_sqsum(vb, ps)
    assert torch.equal(ps, pb)                   # bitwise-identical partials
    # run-to-run determinism of both
    vc, fc, gc, fic, pc = fused()
    assert torch.equal(fc, fb) and torch.equal(pc, pb)
    ps2 = torch.full((n,), GUARD, device=DEV)
    ext.multi_tensor_sqsum(vc, ps2)
    assert torch.equal(ps2, ps)
    assert torch.equal(_finalize(ext, pb, n, 1.0), _finalize(ext, pc, n, 1.0))


# --------------------------------------------------- 4. lazy equals in place ---

@pytest.mark.parametrize("nesterov", [0.0, 1.0])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_lazy_clip_equals_in_place(nesterov, wd):
    ext = _ext()
    sizes = [CH + 1, 7, 4, 1, 0]
    g = torch.Generator().manual_seed(41)
    p0 = [torch.randn(n, generator=g) for n in sizes]
    pa, fpa, gpa = _pack(p0, 1)
    pb, fpb, gpb = _pack(p0, 1)
    ba, fba, gba = _pack([torch.zeros(n) for n in sizes], 2)
    bb, fbb, gbb = _pack([torch.zeros(n) for n in sizes], 2)
    fi = torch.zeros(1, device=DEV)
    for step in range(5):
        grads = [torch.randn(n, generator=g) for n in sizes]
        c = torch.tensor([0.37 / (step + 1)], device=DEV)
        ga_, fga, gga = _pack(grads, 3)
        gb_, fgb, ggb = _pack(grads, 3)
        fga_before = fga.clone()
        ext.fused_sgd(pa, ga_, ba, 0.1, 0.9, wd, nesterov, fi, c)
        ext.multi_tensor_scale(gb_, c, fi)
        ext.fused_sgd(pb, gb_, bb, 0.1, 0.9, wd, nesterov, fi, None)
        assert torch.equal(fpa, fpb), step       # params (+ guards)
        assert torch.equal(fba, fbb), step       # momentum buffers
        assert torch.equal(fga, fga_before)      # lazy: gradients kept
        assert _guards_intact(fgb, ggb)
    assert _guards_intact(fpa, gpa) and _guards_intact(fba, gba)
    assert not torch.equal(fpa.cpu()[~gpa], torch.cat(p0))       # it stepped


def test_momentum_free_lazy_clip():
    ext = _ext()
    p0 = [torch.ones(CH + 1), torch.ones(7)]
    pa, fpa, _ = _pack(p0, 1)
    g_, _, _ = _pack([torch.full((CH + 1,), 2.0), torch.full((7,), 2.0)], 2)
    c = torch.tensor([0.25], device=DEV)
    ext.fused_sgd(pa, g_, [], 1.0, 0.0, 0.0, 0.0, None, c)
    assert all(bool((v == 0.5).all()) for v in pa)   # 1 - 1.0 * (2 * 0.25)


# ------------------------------------------------------ 5. overflow interplay ---

def test_overflow_interplay():
    ext = _ext()
    g = torch.Generator().manual_seed(51)
    cpu = [torch.randn(CH + 1, generator=g), torch.randn(7, generator=g)]
    cpu[0][CH - 3] = float("inf")
    views, dflat, guard = _pack(cpu, 1)
    n = _nchunks(cpu)
    fi = torch.zeros(1, device=DEV)
    partials = torch.zeros(n, device=DEV)
    stats0 = [1.5, 2.5, 1.0, 2.0]
    stats = torch.tensor(stats0, device=DEV)
    ext.multi_tensor_unscale(views, fi, 0.5, partials)
    out = torch.full((2,), -1.0, device=DEV)
    ext.norm_finalize(partials, n, 1.0, fi, out, stats)
    assert float(fi) == 1.0
    assert not math.isfinite(float(out[0]))
    assert float(out[1]) == 1.0
    assert stats.tolist() == stats0
    # the optimizer step and the in-place scale are device-side no-ops
    p0 = [torch.randn(CH + 1, generator=g), torch.randn(7, generator=g)]
    ps, fps, _ = _pack(p0, 2)
    bs, fbs, _ = _pack([torch.zeros(CH + 1), torch.zeros(7)], 3)
    before_p, before_b, before_g = fps.clone(), fbs.clone(), dflat.clone()
    ext.fused_sgd(ps, views, bs, 0.1, 0.9, 5e-4, 1.0, fi, out[1:2])
    ext.multi_tensor_scale(views, torch.tensor([0.5], device=DEV), fi)
    assert torch.equal(fps, before_p) and torch.equal(fbs, before_b)
    assert torch.equal(dflat, before_g)
    # a non-finite norm without a found_inf flag never yields a NaN either
    partials.fill_(float("inf"))
    out2 = _finalize(ext, partials, n, 1.0)
    assert float(out2[1]) == 1.0


# ----------------------------------------------------- 6. clip formula on device ---

def test_clip_formula_on_device():
    ext = _ext()
    views, _, _ = _pack([torch.full((4,), 3.0)], 1)      # norm exactly 6
    partials = torch.zeros(1, device=DEV)
    ext.multi_tensor_sqsum(views, partials)
    stats = torch.zeros(4, device=DEV)
    fi = torch.zeros(1, device=DEV)
    norm32 = torch.tensor(6.0)
    for max_norm, clipped in [(12.0, False), (6.0, True), (3.0, True)]:
        out = _finalize(ext, partials, 1, max_norm, fi, stats)
        assert float(out[0]) == 6.0
        want = np.float32(float((max_norm / (norm32 + 1e-6)).clamp(max=1.0)))
        got = np.float32(float(out[1]))
        assert abs(got - want) <= np.spacing(want), (max_norm, got, want)
        assert (got < 1.0) == clipped
        if not clipped:
            assert got == 1.0
    assert stats.tolist() == [18.0, 6.0, 2.0, 3.0]
    # max_norm == 0: measure only
    assert float(_finalize(ext, partials, 1, 0.0)[1]) == 1.0


# ------------------------------------------- amp branches against the CPU ---

@pytest.mark.parametrize("mode", ["async", "async_inplace", "sync", "O0"])
def test_amp_branches_match_cpu_formula(mode, monkeypatch):
    """Every scale_loss branch on the GPU (lazy, DDPX_CLIP_FUSED=0,
    DDPX_SYNC_AMP=1, amp off) against the CPU path on the same gradients.
    g = w * scale is unscaled exactly (power-of-two scale), so only the norm
    (1e-5, as above) and the fp32 coefficient can differ."""
    from ddp_tricks_amd import amp
    from ddp_tricks_amd.ops.optim import FusedSGD
    monkeypatch.delenv("DDPX_SYNC_AMP", raising=False)
    monkeypatch.delenv("DDPX_CLIP_FUSED", raising=False)
    if mode == "sync":
        monkeypatch.setenv("DDPX_SYNC_AMP", "1")
    if mode == "async_inplace":
        monkeypatch.setenv("DDPX_CLIP_FUSED", "0")
    sizes = (CH + 1, 7, 1)

    def run(dev):
        amp._state.__init__()
        g = torch.Generator().manual_seed(61)
        ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(dev))
              for n in sizes]
        ws = [torch.randn(n, generator=g).to(dev) for n in sizes]
        opt = FusedSGD(ps, lr=0.5, momentum=0.9, nesterov=True)
        _, opt = amp.initialize(None, opt, max_grad_norm=0.5,
                                opt_level="O0" if mode == "O0" else "O1")
        norms, lazy = [], []
        for _ in range(2):
            opt.zero_grad()
            loss = sum((p * w).sum() for p, w in zip(ps, ws))
            with amp.scale_loss(loss, opt) as sl:
                sl.backward()
            lazy.append(amp.pending_grad_scale() is not None)
            norms.append(float(amp.last_grad_norm()))
            opt.step()
        stats = amp.pop_grad_norm_stats()
        amp._state.__init__()
        return [p.detach().cpu() for p in ps], norms, lazy, stats

    p_gpu, n_gpu, lazy, s_gpu = run(DEV)
    p_cpu, n_cpu, _, s_cpu = run(torch.device("cpu"))
    assert lazy == [mode == "async"] * 2
    for a, b in zip(n_gpu, n_cpu):
        assert b > 100 and abs(a - b) <= 1e-5 * b
    assert s_gpu["steps"] == s_cpu["steps"] == 2
    assert s_gpu["clipped_frac"] == s_cpu["clipped_frac"] == 1.0
    for a, b in zip(p_gpu, p_cpu):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------ 7. end to end ---

MAX_NORM = 1e-3

_CHILD = r"""
import json, sys
import torch
from ddp_tricks_amd import amp, same_seeds
from ddp_tricks_amd.models.toy_net import Toy_Net
from ddp_tricks_amd.ops import load_extension
from ddp_tricks_amd.ops.functional import cross_entropy_loss
from ddp_tricks_amd.ops.optim import FusedSGD
from ddp_tricks_amd.utils.lookahead import Lookahead

out_path, max_norm = sys.argv[1], float(sys.argv[2])
load_extension(required=True)
dev = torch.device("cuda:0")
same_seeds(42)
model = Toy_Net().to(dev)
opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
la = Lookahead(opt, k=2, alpha=0.5)
model, la = amp.initialize(model, la, opt_level="O1", max_grad_norm=max_norm)
g = torch.Generator().manual_seed(7)
x = torch.rand(64, 1, 28, 28, generator=g).to(dev)
t = torch.randint(0, 10, (64,), generator=g).to(dev)
model.train()
norms, lazy = [], []
for _ in range(3):
    la.zero_grad()
    out = model(x)
    loss = cross_entropy_loss(out, t) / out.shape[0]
    with amp.scale_loss(loss, la) as scaled:
        scaled.backward()
    lazy.append(amp.pending_grad_scale() is not None)
    norms.append(amp.last_grad_norm().clone())
    la.step()
stats = amp.pop_grad_norm_stats()
torch.save({"params": {k: v.detach().cpu() for k, v in
                       model.state_dict().items()},
            "norms": torch.stack(norms).cpu(), "lazy": lazy,
            "stats": stats}, out_path)
"""


def _run_child(tmp_path, name, fused):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / f"{name}.pt")
    env = dict(os.environ)
    env.pop("DDPX_SYNC_AMP", None)
    if fused:
        env.pop("DDPX_CLIP_FUSED", None)
    else:
        env["DDPX_CLIP_FUSED"] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD, out, str(MAX_NORM)],
                       cwd=repo, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(out, weights_only=False)


@pytest.mark.timeout(300)
def test_e2e_lazy_equals_in_place_and_cpu_norm(tmp_path):
    lazy = _run_child(tmp_path, "lazy", fused=True)
    inpl = _run_child(tmp_path, "inplace", fused=False)
    assert lazy["lazy"] == [True] * 3 and inpl["lazy"] == [False] * 3
    for d in (lazy, inpl):                       # every step clipped
        assert d["stats"]["steps"] == 3 and d["stats"]["clipped_frac"] == 1.0
    assert torch.equal(lazy["norms"], inpl["norms"])
    for k in lazy["params"]:
        assert torch.equal(lazy["params"][k], inpl["params"][k]), k
    assert lazy["stats"] == inpl["stats"]

    # step-1 norm against the CPU fp32 oracle of the same step; 5% relative
    # is what test_gpu_step_matches_cpu_oracle grants bf16-computed values
    from ddp_tricks_amd import amp, same_seeds
    from ddp_tricks_amd.models.toy_net import Toy_Net
    from ddp_tricks_amd.ops.functional import (clear_weight_cache,
                                               cross_entropy_loss)
    from ddp_tricks_amd.ops.optim import FusedSGD
    amp._state.__init__()
    clear_weight_cache()
    same_seeds(42)
    model = Toy_Net()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    model, opt = amp.initialize(model, opt, opt_level="O1",
                                max_grad_norm=MAX_NORM)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(64, 1, 28, 28, generator=g)
    t = torch.randint(0, 10, (64,), generator=g)
    model.train()
    opt.zero_grad()
    out = model(x)
    loss = cross_entropy_loss(out, t) / out.shape[0]
    with amp.scale_loss(loss, opt) as scaled:
        scaled.backward()
    want = float(amp.last_grad_norm())
    amp._state.__init__()
    got = float(lazy["norms"][0])
    assert want > MAX_NORM
    assert abs(got - want) <= 0.05 * want, (got, want)
