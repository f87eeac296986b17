"""Fused BatchNorm+ReLU+MaxPool2d(2) kernels (bn_fwd_train_pool2 /
bn_bwd_pool2) against the unfused HIP pair they replace, against an fp32
torch autograd reference, and through the module routing (conv_bn pool=).
All tests @pytest.mark.gpu — they need an MI355X."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")
CL = torch.channels_last

# (N, C, H, W): baseline; C/8=64 -> four walkers and fewer pooled rows than
# walkers x splits; C/8=3 -> block 255, non-square; the conv2 junction's
# spatial shape (more than one block in every kernel)
SHAPES = [(4, 64, 8, 8), (2, 512, 4, 4), (3, 24, 6, 10), (8, 128, 24, 24)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _close(a, b, rel, atol, name=""):
    a = a.float()
    b = b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    print(f"{name}: err={err:.3e} scale={scale:.3e} "
          f"bound={atol + rel * scale:.3e}")
    assert err <= atol + rel * scale, f"{name}: err={err} scale={scale}"


_CASES = {}


def _case(shape):
    """Inputs plus the unfused and fused HIP results for one shape,
    computed once and shared (read-only) by the tests."""
    if shape in _CASES:
        return _CASES[shape]
    N, C, H, W = shape
    torch.manual_seed(100 + SHAPES.index(shape))
    x = torch.randn(N, C, H, W, device=DEV).to(torch.bfloat16) \
        .contiguous(memory_format=CL)
    g = torch.randn(C, device=DEV).abs() + 0.5
    b = torch.randn(C, device=DEV)
    dyp = torch.randn(N, C, H // 2, W // 2, device=DEV).to(torch.bfloat16) \
        .contiguous(memory_format=CL)
    c = {"x": x, "g": g, "b": b, "dyp": dyp}
    # unfused pair (the parent's code)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y, sm, si, mask = ext.bn_fwd_train(x, g, b, rm, rv, 0.1, 1e-5, True)
    yp, idx = ext.maxpool2x2_fwd(y)
    dy_full = ext.maxpool2x2_bwd(dyp, idx, H, W)
    dx, dg, db = ext.bn_bwd(x, dy_full, g, sm, si, mask, True)
    c["unfused"] = dict(yp=yp, idx=idx, sm=sm, si=si, rm=rm, rv=rv,
                        dx=dx, dg=dg, db=db)
    # fused
    rm2, rv2 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    yp2, sm2, si2, code = ext.bn_fwd_train_pool2(x, g, b, rm2, rv2, 0.1, 1e-5)
    dx2, dg2, db2 = ext.bn_bwd_pool2(x, dyp, g, sm2, si2, code)
    c["fused"] = dict(yp=yp2, code=code, sm=sm2, si=si2, rm=rm2, rv=rv2,
                      dx=dx2, dg=dg2, db=db2)
    torch.cuda.synchronize()
    _CASES[shape] = c
    return c


# ------------------------------------------------- 1. forward, bit-exact ---

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fwd_bit_exact(shape):
    c = _case(shape)
    u, f = c["unfused"], c["fused"]
    assert f["yp"].shape == u["yp"].shape
    assert f["yp"].is_contiguous(memory_format=CL)
    assert torch.equal(f["yp"], u["yp"])
    assert f["code"].shape == u["idx"].shape
    assert torch.equal(f["code"] & 3, u["idx"])
    assert int(f["code"].max()) <= 7
    for k in ("sm", "si", "rm", "rv"):
        assert torch.equal(f[k], u[k]), k


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fwd_bit_exact_pre_stats(shape):
    """Same with the statistics handed in as [2][C][S] partial sums (what
    the producing conv's epilogue emits)."""
    c = _case(shape)
    x, g, b = c["x"], c["g"], c["b"]
    N, C, H, W = shape
    rows = x.float().permute(0, 2, 3, 1).reshape(-1, C)
    parts = torch.tensor_split(rows, 3)
    pre = torch.stack([torch.stack([p.sum(0) for p in parts], 1),
                       torch.stack([(p * p).sum(0) for p in parts], 1)])
    pre = pre.contiguous()
    assert pre.shape == (2, C, 3)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y, sm, si, mask = ext.bn_fwd_train(x, g, b, rm, rv, 0.1, 1e-5, True,
                                       None, pre)
    yp, idx = ext.maxpool2x2_fwd(y)
    rm2, rv2 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    yp2, sm2, si2, code = ext.bn_fwd_train_pool2(x, g, b, rm2, rv2, 0.1,
                                                 1e-5, pre)
    assert torch.equal(yp2, yp)
    assert torch.equal(code & 3, idx)
    assert torch.equal(sm2, sm) and torch.equal(si2, si)
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv)


def test_code_bit2_is_the_relu_mask_bit():
    """Bit 2 of the code is the winner's pre-rounding f > 0 — the bit
    k_bn_apply_v8 puts in its packed mask at the winner's position."""
    shape = SHAPES[0]
    c = _case(shape)
    N, C, H, W = shape
    x, g, b = c["x"], c["g"], c["b"]
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    _, _, _, mask = ext.bn_fwd_train(x, g, b, rm, rv, 0.1, 1e-5, True)
    # mask: [M, C/8] bytes, bit j = channel 8*c8 + j  ->  [N, H, W, C] bool
    bits = (mask.to(torch.int32).view(N, H, W, C // 8, 1)
            >> torch.arange(8, device=DEV, dtype=torch.int32)) & 1
    bits = bits.reshape(N, H, W, C)
    code = c["fused"]["code"].long()               # [N, Ho, Wo, C]
    arg = code & 3
    win = bits.view(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4) \
        .reshape(N, H // 2, W // 2, C, 4).long()
    want = win.gather(-1, arg.unsqueeze(-1)).squeeze(-1)
    assert torch.equal((code >> 2) & 1, want)


def test_rejects_odd_extents_and_layout():
    C = 64
    g = torch.ones(C, device=DEV)
    b = torch.zeros(C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    x = torch.randn(2, C, 7, 8, device=DEV).to(torch.bfloat16) \
        .contiguous(memory_format=CL)
    with pytest.raises(RuntimeError, match="even H and W"):
        ext.bn_fwd_train_pool2(x, g, b, rm, rv, 0.1, 1e-5)
    x = torch.randn(2, C, 8, 8, device=DEV).to(torch.bfloat16)   # NCHW
    with pytest.raises(RuntimeError, match="channels_last"):
        ext.bn_fwd_train_pool2(x, g, b, rm, rv, 0.1, 1e-5)
    x = torch.randn(2, 12, 8, 8, device=DEV).to(torch.bfloat16) \
        .contiguous(memory_format=CL)
    with pytest.raises(RuntimeError, match="C%8"):
        ext.bn_fwd_train_pool2(x, g[:12], b[:12], rm[:12], rv[:12], 0.1, 1e-5)


# ------------------------------- 2. backward vs the unfused composition ---

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bwd_matches_unfused(shape):
    """maxpool2x2_bwd -> bn_bwd is the parent's code; the argmax is
    identical (test_fwd_bit_exact), so only the fp32 summation order of the
    partials differs: the gates of test_bn1pass_matches_twopass."""
    c = _case(shape)
    u, f = c["unfused"], c["fused"]
    assert f["dx"].shape == c["x"].shape
    assert f["dx"].is_contiguous(memory_format=CL)
    _close(f["dg"], u["dg"], rel=1e-4, atol=1e-3, name=f"dgamma {shape}")
    _close(f["db"], u["db"], rel=1e-4, atol=1e-3, name=f"dbeta {shape}")
    _close(f["dx"], u["dx"], rel=1e-2, atol=1e-2, name=f"dx {shape}")


# ------------------------------------ 3. backward vs fp32 torch autograd ---

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bwd_matches_fp32_autograd(shape):
    """Reference: batch_norm -> relu -> straight-through round to bf16 ->
    max_pool2d(2) in fp32 on the same bf16-quantised inputs; tolerances of
    test_bn2d_fwd_bwd.  A last-bit fp32 difference can flip the argmax of
    a window whose top two values nearly tie, so dx leaves out windows
    whose reference top value is positive and whose top two fp32 values
    differ by at most 2^-6 relative — at most 3 % of the windows (asserted).
    dgamma/dbeta are checked over all windows."""
    c = _case(shape)
    N, C, H, W = shape
    xf = c["x"].float().detach().requires_grad_(True)
    g2 = c["g"].detach().clone().requires_grad_(True)
    b2 = c["b"].detach().clone().requires_grad_(True)
    y = F.batch_norm(xf, None, None, g2, b2, True, 0.1, 1e-5).relu()
    yd = y.detach()
    yq = y + (yd.to(torch.bfloat16).float() - yd)
    F.max_pool2d(yq, 2).backward(c["dyp"].float())

    win = yd.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5) \
        .reshape(N, C, H // 2, W // 2, 4)
    top = win.topk(2, dim=-1).values
    t1, t2 = top[..., 0], top[..., 1]
    excl = (t1 > 0) & ((t1 - t2) <= 2.0 ** -6 * t1)
    share = excl.float().mean().item()
    print(f"excluded near-tie windows {shape}: {100 * share:.2f} %")
    assert share <= 0.03, share
    keep = (~excl).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)

    f = c["fused"]
    _close(f["dg"], g2.grad, rel=2e-2, atol=0.1, name=f"dgamma {shape}")
    _close(f["db"], b2.grad, rel=2e-2, atol=0.1, name=f"dbeta {shape}")
    _close(f["dx"].float() * keep, xf.grad * keep, rel=5e-2, atol=2e-2,
           name=f"dx {shape}")


# ------------------------------------------- 4. routing through modules ---

def _graph_has(out, name):
    seen, stack = set(), [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if name in type(fn).__name__:
            return True
        stack.extend(nf for nf, _ in fn.next_functions)
    return False


def _toy_step(model, x, t):
    from ddp_tricks_amd.ops.functional import cross_entropy_loss
    for p in model.parameters():
        p.grad = None
    out = model(x)
    cross_entropy_loss(out, t).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return out, grads


def test_toy_net_routing(monkeypatch):
    """Toy_Net train step, DDPX_BNPOOL=1 against =0 on the same weights and
    batch.  The forward is bit-preserving, so the logits are equal; the
    gradients differ by the BN-backward summation order at the two
    junctions only.  BN weights/biases: the gates of (2).  Conv and linear
    parameters: rel=2e-2 like the conv/linear wgrad tests, with atol=1e-3
    (those tests' atol of 0.5-1.0 is sized for O(100) gradients; here the
    mean-CE gradients are O(1e-2), and the parameters in front of a BN see
    a pure rounding-noise bias gradient that needs an absolute floor)."""
    from ddp_tricks_amd import same_seeds
    from ddp_tricks_amd.models.toy_net import Toy_Net
    for k in ("DDPX_BN1PASS", "DDPX_BNFUSE"):
        monkeypatch.delenv(k, raising=False)
    same_seeds(42)
    model = Toy_Net().to(DEV).train()
    x = torch.rand(8, 1, 28, 28, device=DEV)
    t = torch.randint(0, 10, (8,), device=DEV)
    keys_before = list(model.state_dict().keys())

    monkeypatch.setenv("DDPX_BNPOOL", "0")
    out0, g0 = _toy_step(model, x, t)
    assert not _graph_has(out0, "BatchNormReluPool2")
    monkeypatch.setenv("DDPX_BNPOOL", "1")
    out1, g1 = _toy_step(model, x, t)
    assert _graph_has(out1, "BatchNormReluPool2")
    assert not _graph_has(out1, "MaxPool2x2")
    # the opt-ins that need the full-resolution activation win
    monkeypatch.setenv("DDPX_BN1PASS", "1")
    assert not _graph_has(model(x), "BatchNormReluPool2")
    monkeypatch.delenv("DDPX_BN1PASS")

    assert list(model.state_dict().keys()) == keys_before
    assert torch.equal(out1, out0)
    bn_keys = {f"{n}.{p}" for n, m in model.named_modules()
               if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)
               for p in ("weight", "bias")}
    for k in g0:
        if k in bn_keys:
            _close(g1[k], g0[k], rel=1e-4, atol=1e-3, name=k)
        else:
            _close(g1[k], g0[k], rel=2e-2, atol=1e-3, name=k)


def test_odd_extent_falls_back(monkeypatch):
    """(2,64,7,9) BN->pool pair: the last row/column belongs to no window
    but still takes part in the statistics and dx, so DDPX_BNPOOL=1 must
    take exactly the unfused path."""
    from ddp_tricks_amd.ops.functional import conv_bn
    from ddp_tricks_amd.ops.modules import BatchNorm2d, Conv2d, MaxPool2d
    torch.manual_seed(7)
    conv = Conv2d(8, 64, 3).to(DEV)
    bn = BatchNorm2d(64, fuse_relu=True).to(DEV).train()
    pool = MaxPool2d(2)
    x = torch.randn(2, 8, 9, 11, device=DEV).to(torch.bfloat16) \
        .contiguous(memory_format=CL)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("DDPX_BNPOOL", flag)
        xi = x.clone().requires_grad_(True)
        for p in list(conv.parameters()) + list(bn.parameters()):
            p.grad = None
        out = conv_bn(conv, bn, xi, pool=pool)
        assert out.shape == (2, 64, 3, 4)
        assert not _graph_has(out, "BatchNormReluPool2")
        out.float().square().sum().backward()
        res[flag] = [out.detach(), xi.grad] + [
            p.grad.clone() for p in list(conv.parameters())
            + list(bn.parameters())]
    for a, b in zip(res["0"], res["1"]):
        assert torch.equal(a, b)
    # and the fallback computes a floor-mode pool of the BN output
    with torch.no_grad():
        ref = F.max_pool2d(conv_bn(conv, bn, x).float(), 2)
    assert torch.equal(res["1"][0].float(), ref)


def test_eval_mode_identical(monkeypatch):
    from ddp_tricks_amd import same_seeds
    from ddp_tricks_amd.models.toy_net import Toy_Net
    same_seeds(43)
    model = Toy_Net().to(DEV).eval()
    x = torch.rand(8, 1, 28, 28, device=DEV)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("DDPX_BNPOOL", flag)
        with torch.no_grad():
            outs.append(model(x))
    assert torch.equal(outs[0], outs[1])
