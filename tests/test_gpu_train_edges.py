"""GPU parity of the training kernels where the launchers change kernel and where the inputs of the other op-level
tests (batch 2-4, square images, N(0,1) values) cannot see an indexing or conditioning error: the row-count branches
of the normalisation backward passes and the column sums, every attention-backward and point-attention path (the
vector-ALU fallbacks in a fresh child process, tests/train_fallback_child.py), the MiDaS loss on ragged / tiny /
negative maps, the seen-surface geometry on non-square crops with a full 3x3 intrinsics matrix, and gradient clipping.

Reference: torch on the CPU in float64, on the same fp32 input values upcast.  Comparison: `close` of
tests/test_gpu_train_ops.py (max error over the reference's scale) at the tolerance the existing test of the same op
uses.  The constants marked "measured" are max(that tolerance, 4 x the error of fp32 CPU torch against the float64
reference on the same input); tests/test_train_edge_refs.py recomputes that noise on the CPU and pins them.

The builders / references below run on the CPU alone (the CPU module and the child script import them)."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_train_ops import close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64

FWD, NORM_GRAD = 2e-5, 1e-4
LN_TOL = dict(forward=FWD, dx=FWD, dgamma=FWD, dbeta=FWD)
BN_TOL = dict(forward=FWD, dx=NORM_GRAD, dgamma=NORM_GRAD, dbeta=NORM_GRAD, dres=FWD, running_mean=FWD, running_var=FWD)
GN_TOL = dict(forward=FWD, dx=NORM_GRAD, dgamma=NORM_GRAD, dbeta=NORM_GRAD, dres=FWD)
ATT_TOL = dict(forward=FWD, dqkv=FWD)
PA_TOL = dict(forward=FWD, dqkv_points=FWD, dqkv_latent=FWD, probs=FWD)
SEEN_VAL, SEEN_GRAD = 5e-5, 2e-4
MIDAS_LOSS, MIDAS_GRAD = 2e-5, 2e-4
ADAMW = 1e-6

# ---- measured constants: max(table value, 4 x fp32-CPU-torch error against float64 on the same input) ----
# x = 64 + 0.5 randn, fp32 torch noise of each tensor's scale:
#   LayerNorm 5516x768 (F.layer_norm): forward 5.67e-6, dx 1.39e-6, dgamma 8.15e-6, dbeta 5.1e-7
#     -> 4 x 5.67e-6 = 2.27e-5 and 4 x 8.15e-6 = 3.26e-5 exceed the table's 2e-5; dx and dbeta keep it;
#   BatchNorm 1x32x33x16 (F.batch_norm): forward 1.93e-6, dx 6.1e-7, dgamma 5.99e-6, dbeta 3.4e-7, running stats 1.1e-7;
#   GroupNorm 1x32x32x32 (group_norm_two_pass below): forward 1.79e-6, dx 2.7e-7, dgamma 5.69e-6, dbeta 1.5e-7
#     -> 4 x noise stays below every table value of the two: the table holds.
LN_ILL_TOL = dict(LN_TOL, forward=2.3e-5, dgamma=3.3e-5)
BN_ILL_TOL = dict(BN_TOL)
GN_ILL_TOL = dict(GN_TOL)
# qkv x 4 (logits of +-40): fp32 torch noise at the worst of the three shapes forward 4.82e-6, gradient 3.26e-6 of scale
# -> 4 x 4.82e-6 = 1.93e-5, below the table value.
ATT_BIG_TOL = dict(ATT_TOL)
# point attention on inputs x 4: fp32 torch noise forward 3.03e-6, point gradient 4.76e-6, latent gradient 4.45e-6,
# probabilities 2.04e-6 of scale -> 4 x 4.76e-6 = 1.90e-5, below the table value.
PA_BIG_TOL = dict(PA_TOL)
# d_intr entry by entry, relative to the entry: the fp32 oracle (oracle/frontend_ref under train_ref.differentiable())
# against float64 is off by up to 5.72e-5 of an entry over the four crops and the three losses -> 4 x 5.72e-5 = 2.29e-4,
# above the table's 2e-4.
D_INTR_ENTRY_TOL = 2.3e-4
# FusedAdamW.grad_norm() and the norms the clipping calls return (no table value): torch.nn.utils.clip_grad_norm_ in fp32
# against the float64 norm is off by up to 2.24e-7 over every norm asserted below (the seven tensors together 5.1e-8, each
# alone up to 2.24e-7 at (40000,), the five draws of the clipping tests up to 1.55e-7) -> 4 x 2.24e-7 = 8.96e-7.
GRAD_NORM_TOL = 9.0e-7


def relerr(got, want):
    """The figure `close` bounds: max error over the reference's scale."""
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape
    return float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)


def compare(got, want, tol, what=""):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in sorted(want):
        print("%s %s: %.3e (tolerance %.1e)" % (what, k, relerr(got[k], want[k]), tol[k]))
    for k in sorted(want):
        close(got[k], want[k], rtol=tol[k], what="%s %s" % (what, k))


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def _cuda_leaf(t):
    return t.detach().clone().cuda().requires_grad_(True)


# =====================================================================================================
# A. row-count branches
# =====================================================================================================
LN_CASES = [(4096, 64), (4097, 64), (4099, 100), (5516, 768), (37, 40), (3, 1024), (1, 64)]
LN_ILL_CASE = (5516, 768)


def ln_inputs(rows, C, ill=False):
    g = torch.Generator().manual_seed(rows * 7 + C)
    x = torch.randn(rows, C, generator=g)
    x = 64 + 0.5 * x if ill else x * 2 + 0.5
    return dict(x=x, gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g),
                gy=torch.randn(rows, C, generator=g), gpass=torch.randn(rows, C, generator=g))


def ln_reference(inp, fork, dtype=F64):
    x, ga, be = [_leaf(inp[k], dtype) for k in ("x", "gamma", "beta")]
    y = F.layer_norm(x, (x.shape[-1],), ga, be, 1e-6)
    loss = (y * inp["gy"].to(dtype)).sum()
    if fork:
        loss = loss + (x * inp["gpass"].to(dtype)).sum()
    loss.backward()
    return dict(forward=y.detach(), dx=x.grad, dgamma=ga.grad, dbeta=be.grad)


def ln_gpu(inp, fork):
    from zeroshape_amd.nn import autograd as A
    x, ga, be = [_cuda_leaf(inp[k]) for k in ("x", "gamma", "beta")]
    if fork:
        y, xp = A.layer_norm(x, ga, be, 1e-6, fork=True)
        loss = (y * inp["gy"].cuda()).sum() + (xp * inp["gpass"].cuda()).sum()
    else:
        y = A.layer_norm(x, ga, be, 1e-6)
        loss = (y * inp["gy"].cuda()).sum()
    loss.backward()
    return dict(forward=y.detach(), dx=x.grad, dgamma=ga.grad, dbeta=be.grad)


@pytest.mark.parametrize("fork", [False, True], ids=["plain", "fork"])
@pytest.mark.parametrize("rows,C", LN_CASES)
def test_layer_norm_backward_row_branches(rows, C, fork):
    """4 rows per workgroup up to 4096 rows, 16 above; C that is no multiple of 64; one row; the pass-through gradient
    of fork=True added inside the kernel that writes dx (zs_layer_norm_bwd_add)."""
    inp = ln_inputs(rows, C)
    compare(ln_gpu(inp, fork), ln_reference(inp, fork), LN_TOL, "layer_norm %dx%d" % (rows, C))


def test_layer_norm_backward_limit():
    from zeroshape_amd import _lib
    inp = ln_inputs(3, 1025)
    with pytest.raises(_lib.ZeroShapeHipError):
        ln_gpu(inp, False)


# (B, H, W, C) channels-last, relu, residual: rows = B H W at and around the fused kernel's 1024 and the chunk cap's 65536
BN_CASES = [((1, 32, 32, 16), True, True), ((1, 32, 33, 16), False, False), ((1, 1025, 1, 8), True, False),
            ((1, 65536, 1, 4), False, True), ((1, 65537, 1, 8), True, True), ((1, 70000, 1, 12), False, False)]
BN_ILL_CASE = ((1, 32, 33, 16), False, True)


def bn_inputs(shape, res, ill=False):
    C = shape[-1]
    g = torch.Generator().manual_seed(shape[1] * 3 + shape[2] + C)
    x = torch.randn(shape, generator=g)
    x = 64 + 0.5 * x if ill else x * 1.5 + 0.3
    return dict(x=x, res=torch.randn(shape, generator=g) if res else None, gamma=torch.rand(C, generator=g) + 0.5,
                beta=torch.randn(C, generator=g) * 0.2, running_mean=torch.randn(C, generator=g) * 0.1,
                running_var=torch.rand(C, generator=g) + 0.5, gy=torch.randn(shape, generator=g))


def bn_reference(inp, relu, dtype=F64):
    C = inp["x"].shape[-1]
    x, ga, be = [_leaf(inp[k], dtype) for k in ("x", "gamma", "beta")]
    r = None if inp["res"] is None else _leaf(inp["res"], dtype)
    rm, rv = inp["running_mean"].to(dtype).clone(), inp["running_var"].to(dtype).clone()
    y = F.batch_norm(x.reshape(-1, C), rm, rv, ga, be, True, 0.1, 1e-5).reshape(x.shape)
    if r is not None:
        y = y + r
    y = F.relu(y) if relu else y
    (y * inp["gy"].to(dtype)).sum().backward()
    out = dict(forward=y.detach(), dx=x.grad, dgamma=ga.grad, dbeta=be.grad, running_mean=rm, running_var=rv)
    if r is not None:
        out["dres"] = r.grad
    return out


def bn_gpu(inp, relu):
    from zeroshape_amd.nn import autograd as A
    C = inp["x"].shape[-1]
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(inp["gamma"])
        bn.bias.copy_(inp["beta"])
        bn.running_mean.copy_(inp["running_mean"])
        bn.running_var.copy_(inp["running_var"])
    bn = bn.cuda()
    x = _cuda_leaf(inp["x"])
    r = None if inp["res"] is None else _cuda_leaf(inp["res"])
    y = A.batch_norm_train(x, bn, relu=relu, residual=r)
    (y * inp["gy"].cuda()).sum().backward()
    assert int(bn.num_batches_tracked) == 1
    out = dict(forward=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
               running_var=bn.running_var)
    if r is not None:
        out["dres"] = r.grad
    return out


@pytest.mark.parametrize("shape,relu,res", BN_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_batch_norm_row_branches(shape, relu, res):
    """The fused strip kernel up to 1024 rows, three launches above; more than 65536 rows: the chunk count is capped at
    256 and a chunk holds more than 256 rows."""
    inp = bn_inputs(shape, res)
    compare(bn_gpu(inp, relu), bn_reference(inp, relu), BN_TOL, "batch_norm %s" % (shape,))


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("rows,C", [(1, 5), (255, 64), (257, 70), (131072, 4), (131075, 4)])
def test_column_sum(rows, C, scale):
    """zs_column_sum (bias / token gradients): one chunk, ragged column blocks, the 512-chunk cap (rows > 131072)."""
    from zeroshape_amd.nn import autograd as A
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g) + 0.1
    close(A.column_sum(x.cuda(), scale), x.double().sum(0) * scale, rtol=FWD, what="column_sum %dx%d" % (rows, C))


# (B, H, C, groups), relu, residual: 1 / 2 / 4 / 64 channels per group; 1, 2 and 16 pixel slices, a short last slice
GN_CASES = [((2, 9, 32, 32), True, True), ((1, 8, 128, 32), False, False), ((1, 8, 2048, 32), True, False),
            ((3, 5, 64, 8), False, True), ((1, 32, 32, 32), True, True), ((1, 33, 32, 32), False, False),
            ((28, 8, 64, 32), True, False)]
GN_ILL_CASE = ((1, 32, 32, 32), False, True)


def gn_inputs(cfg, res, ill=False):
    B, H, C, groups = cfg
    g = torch.Generator().manual_seed(B + 10 * H + C + groups)
    x = torch.randn(B, H, H, C, generator=g)                       # channels-last
    x = 64 + 0.5 * x if ill else x * 2 + 0.5
    return dict(x=x, res=torch.randn(B, H, H, C, generator=g) if res else None, gamma=torch.rand(C, generator=g) + 0.5,
                beta=torch.randn(C, generator=g) * 0.2, gy=torch.randn(B, H, H, C, generator=g), groups=groups)


def group_norm_two_pass(x, groups, gamma, beta, eps):
    """GroupNorm over channels-last x in plain torch ops, the variance about the mean (in fp32 F.group_norm on the CPU
    takes E[x^2] - mean^2 and loses the variance of x = 64 + 0.5 randn; in float64 the two agree, pinned by
    tests/test_train_edge_refs.py)."""
    B, H, W, C = x.shape
    xg = x.reshape(B, H * W, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    return ((xg - mean) / torch.sqrt(var + eps)).reshape(B, H, W, C) * gamma + beta


def gn_reference(inp, relu, dtype=F64):
    x, ga, be = [_leaf(inp[k], dtype) for k in ("x", "gamma", "beta")]
    r = None if inp["res"] is None else _leaf(inp["res"], dtype)
    y = group_norm_two_pass(x, inp["groups"], ga, be, 1e-5)
    if r is not None:
        y = y + r
    y = F.relu(y) if relu else y
    (y * inp["gy"].to(dtype)).sum().backward()
    out = dict(forward=y.detach(), dx=x.grad, dgamma=ga.grad, dbeta=be.grad)
    if r is not None:
        out["dres"] = r.grad
    return out


def gn_gpu(inp, relu):
    from zeroshape_amd.nn import autograd as A
    x, ga, be = [_cuda_leaf(inp[k]) for k in ("x", "gamma", "beta")]
    r = None if inp["res"] is None else _cuda_leaf(inp["res"])
    y = A.group_norm(x, ga, be, inp["groups"], 1e-5, relu=relu, residual=r)
    (y * inp["gy"].cuda()).sum().backward()
    out = dict(forward=y.detach(), dx=x.grad, dgamma=ga.grad, dbeta=be.grad)
    if r is not None:
        out["dres"] = r.grad
    return out


@pytest.mark.parametrize("cfg,relu,res", GN_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_group_norm_backward_branches(cfg, relu, res):
    inp = gn_inputs(cfg, res)
    compare(gn_gpu(inp, relu), gn_reference(inp, relu), GN_TOL, "group_norm %s" % (cfg,))


def test_ill_conditioned_statistics():
    """x = 64 + 0.5 randn: mean^2 is 16,000 x the variance - a one-pass fp32 variance would lose every digit."""
    inp = ln_inputs(*LN_ILL_CASE, ill=True)
    compare(ln_gpu(inp, True), ln_reference(inp, True), LN_ILL_TOL, "layer_norm ill")
    shape, relu, res = BN_ILL_CASE
    inp = bn_inputs(shape, res, ill=True)
    compare(bn_gpu(inp, relu), bn_reference(inp, relu), BN_ILL_TOL, "batch_norm ill")
    cfg, relu, res = GN_ILL_CASE
    inp = gn_inputs(cfg, res, ill=True)
    compare(gn_gpu(inp, relu), gn_reference(inp, relu), GN_ILL_TOL, "group_norm ill")


# =====================================================================================================
# B. attention
# =====================================================================================================
ATT_CASES = [(1, 257, 1, 32), (1, 300, 2, 64), (1, 315, 1, 64), (1, 512, 1, 32), (1, 256, 2, 32), (2, 32, 1, 64),
             (1, 1, 1, 32), (1, 3, 2, 32), (2, 197, 2, 64)]
ATT_BIG_CASES = [(2, 197, 2, 64), (1, 300, 1, 32), (2, 65, 2, 32)]
ATT_CHILD_CASES = [(2, 197, 2, 64), (2, 65, 2, 32), (1, 3, 2, 32)]


def attention_inputs(B, L, heads, d, mult=1.0):
    g = torch.Generator().manual_seed(L * 131 + heads * 7 + d)
    C = heads * d
    return dict(qkv=torch.randn(B, L, 3 * C, generator=g) * mult, go=torch.randn(B, L, C, generator=g), heads=heads)


def attention_reference(inp, dtype=F64):
    qkv = _leaf(inp["qkv"], dtype)
    B, L, C3 = qkv.shape
    heads, d = inp["heads"], C3 // 3 // inp["heads"]
    q, k, v = qkv.reshape(B, L, 3, heads, d).permute(2, 0, 3, 1, 4).unbind(0)
    o = (((q @ k.transpose(-2, -1)) * d ** -0.5).softmax(-1) @ v).transpose(1, 2).reshape(B, L, heads * d)
    o.backward(inp["go"].to(dtype))
    return dict(forward=o.detach(), dqkv=qkv.grad)


def attention_gpu(inp):
    from zeroshape_amd.nn import autograd as A
    qkv = _cuda_leaf(inp["qkv"])
    o = A.attention(qkv, inp["heads"])
    o.backward(inp["go"].cuda())
    return dict(forward=o.detach(), dqkv=qkv.grad)


@pytest.mark.parametrize("B,L,heads,d", ATT_CASES)
def test_attention_backward_paths(B, L, heads, d):
    """L > 256: attention_bwd_rows_kernel (315 x 64 is the last L that fits its 160 KB of LDS); L = 256 fills the MFMA
    pass; L = 257, 315, 1, 3, 197: padded LS rows; L = 32, 1: a single key tile."""
    inp = attention_inputs(B, L, heads, d)
    compare(attention_gpu(inp), attention_reference(inp), ATT_TOL, "attention %s" % ((B, L, heads, d),))


def test_attention_backward_limit():
    from zeroshape_amd import _lib
    with pytest.raises(_lib.ZeroShapeHipError):
        attention_gpu(attention_inputs(1, 316, 1, 64))


@pytest.mark.parametrize("B,L,heads,d", ATT_BIG_CASES)
def test_attention_large_logits(B, L, heads, d):
    """qkv x 4: logits of +-40, the max subtraction carries the softmax."""
    inp = attention_inputs(B, L, heads, d, mult=4.0)
    compare(attention_gpu(inp), attention_reference(inp), ATT_BIG_TOL, "attention x4 %s" % ((B, L, heads, d),))


@pytest.mark.parametrize("mult", [1.0, 4.0])
@pytest.mark.parametrize("B,L,heads,d", [(16, 97, 8, 32), (16, 64, 8, 32)])
def test_inference_attention_lds_staged(B, L, heads, d, mult, monkeypatch):
    """ops.attention under f16x3 with B heads >= 128: attention_lds_kernel (keys padded to 224 / 96)."""
    from zeroshape_amd.nn import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", "f16x3")
    inp = attention_inputs(B, L, heads, d, mult=mult)
    want = attention_reference(inp)["forward"]
    with torch.no_grad():
        got = ops.attention(inp["qkv"].cuda(), heads)
    print("ops.attention %s x%g: %.3e" % ((B, L, heads, d), mult, relerr(got, want)))
    close(got, want, rtol=FWD, what="ops.attention")


def test_training_attention_follows_the_training_precision(monkeypatch):
    """A.attention picks its kernel from the TRAINING forward precision (fp32 unless optim.amp), never from the inference
    switch ops.CONV_PRECISION: bit-equal to the fp32 kernel by default and to the split-fp16 one after
    set_forward_precision("f16x3").  33 keys: more than one 32-key tile and a ragged tail."""
    from zeroshape_amd.nn import autograd as A, ops
    from zeroshape_amd.nn.operands import SWITCHES
    heads = 2
    qkv = torch.randn(2, 33, 3 * 64, generator=torch.Generator().manual_seed(33)).cuda()
    with torch.no_grad():
        with monkeypatch.context() as m:
            m.setattr(ops, "CONV_PRECISION", "f32")
            r32 = ops.attention(qkv, heads)
            m.setattr(ops, "CONV_PRECISION", "f16x3")
            r16 = ops.attention(qkv, heads)
    assert not torch.equal(r32, r16), "precondition: the two arithmetics must differ on this input (choose another seed)"
    monkeypatch.setattr(A, "ATT_FWD_SPLIT", True)
    before = SWITCHES.forward
    try:
        A.set_forward_precision("f32")
        assert torch.equal(A.attention(qkv, heads), r32)
        A.set_forward_precision("f16x3")
        assert torch.equal(A.attention(qkv, heads), r16)
    finally:
        A.set_forward_precision(before)


PA_HEADS, PA_D = 8, 32
PA_CASES = [(1, 33, 256), (2, 70, 64), (1, 40, 65), (1, 5, 1), (1, 513, 197)]
PA_NUMERIC_CASE = (2, 300, 197)
PA_CHILD_CASES = [(2, 300, 197), (1, 5, 1), (1, 513, 197)]


def point_attention_inputs(B, M, Ll, mult=1.0, self_dominant=False):
    C = PA_HEADS * PA_D
    g = torch.Generator().manual_seed(M * 17 + Ll)
    qp, ql = torch.randn(B, M, 3 * C, generator=g) * mult, torch.randn(B, Ll, 3 * C, generator=g) * mult
    if self_dominant:
        qp[..., C:2 * C] = 6 * qp[..., :C]                         # self logit 6 |q|^2 / sqrt(32) ~ 34: it owns the row
    return dict(qp=qp, ql=ql, go=torch.randn(B, M, C, generator=g))


def point_attention_reference(inp, dtype=F64):
    """The reference of test_point_attention (tests/test_gpu_train_ops.py) + the head-averaged cross probabilities."""
    heads, d, C = PA_HEADS, PA_D, PA_HEADS * PA_D
    pr, lr = _leaf(inp["qp"], dtype), _leaf(inp["ql"], dtype)
    B, M, Ll = pr.shape[0], pr.shape[1], lr.shape[1]
    sp = lambda t, n: t.reshape(B, n, 3, heads, d).permute(2, 0, 3, 1, 4).unbind(0)   # noqa: E731
    q_p, k_p, v_p = sp(pr, M)
    _, k_l, v_l = sp(lr, Ll)
    cross = (q_p @ k_l.transpose(-2, -1)) * d ** -0.5
    self_ = (q_p * k_p).sum(-1, keepdim=True) * d ** -0.5
    joint = torch.cat([cross, self_], -1).softmax(-1)
    o = (joint[..., :Ll] @ v_l + joint[..., Ll:] * v_p).transpose(1, 2).reshape(B, M, C)
    o.backward(inp["go"].to(dtype))
    return dict(forward=o.detach(), dqkv_points=pr.grad, dqkv_latent=lr.grad, probs=joint[..., :Ll].mean(1).detach())


def point_attention_gpu(inp):
    from zeroshape_amd.nn import autograd as A
    pg, lg = _cuda_leaf(inp["qp"]), _cuda_leaf(inp["ql"])
    o = A.point_attention(pg, lg, PA_HEADS)
    o.backward(inp["go"].cuda())
    B, M, Ll = pg.shape[0], pg.shape[1], lg.shape[1]
    attn = torch.full((B, M, Ll), 7.0, device="cuda")               # overwritten, then accumulated into
    A.point_attention_probs(pg, lg, PA_HEADS, attn, weight=0.25)
    A.point_attention_probs(pg, lg, PA_HEADS, attn, weight=0.75, accumulate=True)
    assert float(lg.grad[..., :PA_HEADS * PA_D].abs().max()) == 0   # latent queries are unused here
    return dict(forward=o.detach(), dqkv_points=pg.grad, dqkv_latent=lg.grad, probs=attn)


@pytest.mark.parametrize("B,M,Ll", PA_CASES)
def test_point_attention_shapes(B, M, Ll):
    """Ll = 256: all eight latent tiles; 65, 1: a ragged / single tile; M = 33, 513: ragged point tiles, two 512-point
    chunks of the latent-gradient partials."""
    inp = point_attention_inputs(B, M, Ll)
    compare(point_attention_gpu(inp), point_attention_reference(inp), PA_TOL, "point_attention %s" % ((B, M, Ll),))


def test_point_attention_limit():
    from zeroshape_amd import _lib
    with pytest.raises(_lib.ZeroShapeHipError):
        point_attention_gpu(point_attention_inputs(1, 5, 257))


@pytest.mark.parametrize("kind", ["x4", "self"])
def test_point_attention_numerics(kind):
    """Inputs x 4; and k_p = 6 q_p, where the point's own logit (~34) dominates the joint softmax row."""
    inp = point_attention_inputs(*PA_NUMERIC_CASE, mult=4.0 if kind == "x4" else 1.0, self_dominant=kind == "self")
    compare(point_attention_gpu(inp), point_attention_reference(inp), PA_BIG_TOL if kind == "x4" else PA_TOL,
            "point_attention " + kind)


# ---- the kernels behind process-wide switches: a fresh child per set of switches ----
CHILD = os.path.join(ROOT, "tests", "train_fallback_child.py")
CHILD_BN_CASES = [((1, 32, 32, 16), True, True), ((3, 5, 5, 8), False, False)]
CHILD_LN_CASES = [(4097, 64), (37, 40)]
_CHILD_DIED = []


def child_cases(mode):
    """name -> (function returning {quantity: error}, {quantity: tolerance}); what tests/train_fallback_child.py runs."""
    cases = {}

    def add(name, gpu, ref, tol, keys=None):
        def run():
            got, want = gpu(), ref()
            return {k: relerr(got[k], want[k]) for k in (keys or sorted(want))}
        cases[name] = (run, {k: tol[k] for k in (keys or sorted(tol))})
    if mode == "valu":
        for c in ATT_CHILD_CASES:
            inp = attention_inputs(*c)
            add("attention_bwd %s" % (c,), lambda i=inp: attention_gpu(i), lambda i=inp: attention_reference(i), ATT_TOL)
        for c in PA_CHILD_CASES:
            inp = point_attention_inputs(*c)
            add("point_attention %s" % (c,), lambda i=inp: point_attention_gpu(i), lambda i=inp: point_attention_reference(i),
                PA_TOL)
    elif mode == "unfused":
        for shape, relu, res in CHILD_BN_CASES:
            inp = bn_inputs(shape, res)
            add("batch_norm %s" % (shape,), lambda i=inp, r=relu: bn_gpu(i, r), lambda i=inp, r=relu: bn_reference(i, r), BN_TOL,
                keys=[k for k in sorted(BN_TOL) if k != "dres" or res])
        for c in CHILD_LN_CASES:
            inp = ln_inputs(*c)
            add("layer_norm fork %s" % (c,), lambda i=inp: ln_gpu(i, True), lambda i=inp: ln_reference(i, True), LN_TOL)
    else:
        raise ValueError(mode)
    return cases


CHILD_ENV = {"valu": {"ZS_ATTN_BWD_VALU": "1", "ZS_POINT_ATTN_VALU": "1"},
             "unfused": {"ZS_BN_FUSED_ROWS": "0", "ZS_TRAIN_FUSE_FORKS": "0"}}


@pytest.mark.parametrize("mode", ["valu", "unfused"])
def test_switched_kernels_in_a_fresh_child(mode):
    """The vector-ALU attention-backward / point-attention kernels (ZS_ATTN_BWD_VALU, ZS_POINT_ATTN_VALU: also the path of
    more than 2,097,120 points) and the three-launch BatchNorm / unfused forks (ZS_BN_FUSED_ROWS=0, ZS_TRAIN_FUSE_FORKS=0).
    The libraries read the switches once per process: each set runs in a child started fresh."""
    assert not _CHILD_DIED, "an earlier child died (%s): nothing more is started" % _CHILD_DIED[0]
    env = dict(os.environ)
    env.update(CHILD_ENV[mode])
    try:
        r = subprocess.run([sys.executable, CHILD, mode], env=env, timeout=180, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append("%s: time limit" % mode)
        pytest.fail("child %s ran into its time limit" % mode)
    if r.returncode != 0:                  # a signal, or an exit after a HIP error: the next child is not started
        _CHILD_DIED.append("%s: exit status %d" % (mode, r.returncode))
    assert r.returncode == 0, "child %s: exit status %d\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["env"] == CHILD_ENV[mode]
    want = child_cases(mode)
    assert sorted(out["errors"]) == sorted(want)
    print(json.dumps(out["errors"], sort_keys=True))
    for name, (_, tol) in want.items():
        assert sorted(out["errors"][name]) == sorted(tol), name
        for k, e in out["errors"][name].items():
            assert e <= tol[k], "%s %s: %.3e > %.1e" % (name, k, e, tol[k])


# =====================================================================================================
# C. MiDaS loss
# =====================================================================================================
MIDAS_SHAPES = [(2, 5, 7), (3, 13, 9), (2, 33, 17), (2, 8, 8), (1, 1, 40), (2, 3, 3)]


def midas_inputs(B, H, W, inverse_depth):
    """rand + 0.3 for inverse depth, randn (negative values reach the medians) for plain depth; mask = rand > 0.25, from
    the first seed that leaves every sample at least four valid pixels (with two or three the fp32 determinant of the
    scale-and-shift fit cancels and the reference itself is ill-conditioned)."""
    seed = 100 * H + W
    while True:
        g = torch.Generator().manual_seed(seed)
        pred, target = torch.rand(B, 1, H, W, generator=g) + 0.3, torch.rand(B, 1, H, W, generator=g) + 0.3
        if not inverse_depth:
            pred, target = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
        mask = (torch.rand(B, 1, H, W, generator=g) > 0.25).float()
        if int(mask.sum((1, 2, 3)).min()) >= 4:
            return dict(pred=pred, target=target, mask=mask, alpha=0.5, scales=4, inverse_depth=inverse_depth)
        seed += 1


def midas_one_valid_pixel():
    """Sample 0 keeps one pixel: det == 0 in the scale-and-shift fit, with alpha > 0."""
    g = torch.Generator().manual_seed(11)
    pred, target = torch.rand(2, 1, 6, 6, generator=g) + 0.3, torch.rand(2, 1, 6, 6, generator=g) + 0.3
    mask = (torch.rand(2, 1, 6, 6, generator=g) > 0.25).float()
    mask[0] = 0
    mask[0, 0, 2, 3] = 1
    return dict(pred=pred, target=target, mask=mask, alpha=0.5, scales=4, inverse_depth=True)


def midas_one_sample_masked():
    g = torch.Generator().manual_seed(12)
    pred, target = torch.rand(3, 1, 9, 11, generator=g) + 0.3, torch.rand(3, 1, 9, 11, generator=g) + 0.3
    mask = (torch.rand(3, 1, 9, 11, generator=g) > 0.25).float()
    mask[1] = 0
    return dict(pred=pred, target=target, mask=mask, alpha=0.3, scales=4, inverse_depth=True)


def midas_reference(inp, dtype=F64):
    from oracle import loss_ref
    p = _leaf(inp["pred"], dtype)
    loss = loss_ref.midas_loss(p, inp["target"].to(dtype), inp["mask"], alpha=inp["alpha"], scales=inp["scales"],
                               inverse_depth=inp["inverse_depth"])
    loss.backward()
    return loss.detach(), p.grad


def midas_check(inp, what):
    from zeroshape_amd.nn import autograd as A
    want_loss, want_grad = midas_reference(inp)
    p = _cuda_leaf(inp["pred"])
    loss = A.midas_loss(p, inp["target"].cuda(), inp["mask"].cuda(), alpha=inp["alpha"], scales=inp["scales"],
                        inverse_depth=inp["inverse_depth"])
    loss.backward()
    print("%s: loss %.6f (reference %.6f), gradient error %.3e" % (what, float(loss), float(want_loss), relerr(p.grad, want_grad)))
    assert bool(torch.isfinite(p.grad).all())
    assert abs(float(loss) - float(want_loss)) <= MIDAS_LOSS * abs(float(want_loss)), what
    close(p.grad, want_grad, rtol=MIDAS_GRAD, what=what + " gradient")
    return p.grad.cpu(), want_grad


@pytest.mark.parametrize("inverse_depth", [True, False], ids=["inverse", "plain"])
@pytest.mark.parametrize("B,H,W", MIDAS_SHAPES)
def test_midas_loss_ragged_and_tiny_maps(B, H, W, inverse_depth):
    """Odd H / W under four scales, maps smaller than the 1024-lane workgroup, one row, 3 x 3; negative values."""
    midas_check(midas_inputs(B, H, W, inverse_depth), "midas %s" % ((B, H, W),))


def test_midas_loss_one_valid_pixel_and_empty_sample():
    got, want = midas_check(midas_one_valid_pixel(), "midas one valid pixel")
    assert float(want[0].abs().max()) == 0 and float(got[0].abs().max()) == 0
    got, want = midas_check(midas_one_sample_masked(), "midas one sample masked")
    assert float(want[1].abs().max()) == 0 and float(got[1].abs().max()) == 0


# =====================================================================================================
# D. seen-surface geometry, non-square
# =====================================================================================================
# (row offset, column offset, H, W, dsp) crops of synthetic.seeded_depth_scene(seed=2, batch=2)
SEEN_CROPS = [(60, 50, 40, 56, 1), (60, 50, 56, 40, 1), (90, 90, 10, 12, 1), (70, 60, 24, 38, 2)]
# Seeds of the upstream gradients.  A d_intr entry is a sum over the pixels that random gradients can make cancel to a
# small fraction of its terms; such an entry is ill-conditioned in the fp32 oracle itself.  The seeds are chosen by the
# oracle's own fp32-against-float64 noise per entry, which tests/test_train_edge_refs.py recomputes and bounds.
SEEN_GRAD_SEEDS = {SEEN_CROPS[0]: 5, SEEN_CROPS[1]: 4, SEEN_CROPS[2]: 3, SEEN_CROPS[3]: 1}


def intr_param2mtx_ref(H, W, params):
    """graph_shape.py:89-113 (oracle/frontend_ref.intr_param2mtx), differentiable, in the dtype of `params`."""
    zoom = torch.pow(torch.tensor(4.0, dtype=params.dtype), torch.tanh(params[:, 0]))
    rows = [torch.stack([1.3875 * W * zoom, torch.zeros_like(zoom), W / 2 + torch.tanh(params[:, 1]) * W / 2], -1),
            torch.stack([torch.zeros_like(zoom), 1.3875 * H * zoom, H / 2 + torch.tanh(params[:, 2]) * H / 2], -1),
            torch.stack([torch.zeros_like(zoom), torch.zeros_like(zoom), torch.ones_like(zoom)], -1)]
    return torch.stack(rows, 1)


def seen_inputs(crop, full_matrix=True):
    from zeroshape_amd import synthetic as syn
    r0, c0, H, W, dsp = crop
    depth, mask, params = [torch.from_numpy(a) for a in syn.seeded_depth_scene(seed=2, batch=2)]
    depth, mask = depth[:, :, r0:r0 + H, c0:c0 + W].contiguous(), mask[:, :, r0:r0 + H, c0:c0 + W].contiguous()
    K = intr_param2mtx_ref(H, W, params)
    if full_matrix:                                                # all nine entries carry a gradient of their own
        K[:, 0, 1], K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = 3, -2, 1e-3, -5e-4
    g = torch.Generator().manual_seed(H * 100 + W + 1000 * SEEN_GRAD_SEEDS[crop])
    return dict(depth=depth, mask=mask, params=params, K=K, dsp=dsp, gs=torch.randn(2, H * W, 3, generator=g),
                gc=torch.randn(2, 3, H // dsp, W // dsp, generator=g))


def seen_surface_ref(depth, K, mask, dsp):
    """unproj_depth -> valid_norm_fac -> normalise, invalid := 0 -> masked_resample (oracle/frontend_ref.seen_surface) in
    the dtype of its inputs and differentiable: the oracle casts inv(K) to float and zeroes in place."""
    B, _, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=depth.dtype), torch.arange(W, dtype=depth.dtype), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(1, -1, 3)
    rays = torch.linalg.inv(K) @ pix.expand(B, -1, -1).transpose(1, 2)
    pts = rays.transpose(1, 2) * depth.reshape(B, H * W, 1)
    sel = (mask > 0.5).reshape(B, -1)
    mean = torch.stack([pts[b][sel[b]].mean(0) for b in range(B)])
    scale = torch.stack([(pts[b][sel[b]] - mean[b]).norm(dim=1).max() for b in range(B)])
    seen = (pts - mean[:, None]) / scale[:, None, None] * sel[..., None].to(depth.dtype)
    seen_map = seen.reshape(B, H, W, 3).permute(0, 3, 1, 2)
    m = (mask > 0.5).to(depth.dtype)
    size = (H // dsp, W // dsp)
    num = F.interpolate(seen_map * m, size, mode="bilinear", align_corners=False)
    den = F.interpolate(m, size, mode="bilinear", align_corners=False)
    keep = (den > 0.5).to(depth.dtype)
    return seen, num / (den + 1.0e-6) * keep, keep, mean, scale


def seen_reference(inp, use=("seen", "coord"), dtype=F64, chained=False):
    d = _leaf(inp["depth"], dtype)
    leaf = _leaf(inp["params"] if chained else inp["K"], dtype)
    K = intr_param2mtx_ref(d.shape[2], d.shape[3], leaf) if chained else leaf
    seen, coord, keep, mean, scale = seen_surface_ref(d, K, inp["mask"].to(dtype), inp["dsp"])
    loss = 0
    if "seen" in use:
        loss = loss + (seen * inp["gs"].to(dtype)).sum()
    if "coord" in use:
        loss = loss + (coord * inp["gc"].to(dtype)).sum()
    loss.backward()
    return dict(seen=seen.detach(), coord=coord.detach(), mask=keep, mean=mean.detach(), scale=scale.detach(),
                d_depth=d.grad, d_leaf=leaf.grad)


def seen_gpu(inp, use=("seen", "coord"), chained=False, mask=None):
    from zeroshape_amd.nn import autograd as A
    d = _cuda_leaf(inp["depth"])
    leaf = _cuda_leaf(inp["params"] if chained else inp["K"])
    K = A.intr_param2mtx(leaf, d.shape[2], d.shape[3]) if chained else leaf
    fn = A.seen_surface_dsp2 if inp["dsp"] == 2 else A.seen_surface
    seen, coord, keep = fn(d, K, (inp["mask"] if mask is None else mask).cuda())
    mean, scale = seen.grad_fn.saved_tensors[3:5]                  # the statistics the backward pass reads
    loss = 0
    if "seen" in use:
        loss = loss + (seen * inp["gs"].cuda()).sum()
    if "coord" in use:
        loss = loss + (coord * inp["gc"].cuda()).sum()
    loss.backward()
    return dict(seen=seen.detach(), coord=coord.detach(), mask=keep, mean=mean, scale=scale, d_depth=d.grad, d_leaf=leaf.grad)


def entry_errors(got, want):
    """|got - want| / |want|, entry by entry."""
    got, want = got.detach().cpu().double(), want.detach().double()
    return ((got - want).abs() / want.abs()).reshape(-1)


def check_seen(got, want, what):
    for k in ("seen", "coord", "mean", "scale"):
        print("%s %s: %.3e" % (what, k, relerr(got[k], want[k])))
        close(got[k], want[k], rtol=SEEN_VAL, what="%s %s" % (what, k))
    assert torch.equal(got["mask"].cpu().double(), want["mask"]), what + " mask"
    print("%s d_depth: %.3e" % (what, relerr(got["d_depth"], want["d_depth"])))
    close(got["d_depth"], want["d_depth"], rtol=SEEN_GRAD, what=what + " d_depth")


@pytest.mark.parametrize("use", [("seen", "coord"), ("seen",), ("coord",)], ids=["both", "seen", "coord"])
@pytest.mark.parametrize("crop", SEEN_CROPS, ids=lambda c: "%dx%d_dsp%d" % c[2:])
def test_seen_surface_non_square_full_intrinsics(crop, use):
    """H != W (x = i % W, y = i / W), a K with nine distinct entries as the leaf: every d_intr entry against its own
    size, not against the largest of the nine; losses that use only one of the two outputs (autograd hands the unused
    one a zero gradient tensor: the d_seen / d_coord == None branches of the backward pass are not reached here)."""
    inp = seen_inputs(crop)
    got, want = seen_gpu(inp, use), seen_reference(inp, use)
    what = "seen_surface %s %s" % (crop, "+".join(use))
    check_seen(got, want, what)
    err = entry_errors(got["d_leaf"], want["d_leaf"])
    print("%s d_intr entry errors: %s" % (what, " ".join("%.2e" % e for e in err.tolist())))
    assert float(err.max()) <= D_INTR_ENTRY_TOL, (what, err.reshape(-1, 3, 3))


@pytest.mark.parametrize("crop", SEEN_CROPS, ids=lambda c: "%dx%d_dsp%d" % c[2:])
def test_seen_surface_non_square_chained_intrinsics(crop):
    """A.intr_param2mtx(params, H, W) at H != W in front: d_params (g[0] f W + g[4] f H would pass with H and W swapped
    on a square image)."""
    from zeroshape_amd.nn import autograd as A
    inp = seen_inputs(crop, full_matrix=False)
    H, W = inp["depth"].shape[2:]
    close(A.intr_param2mtx(inp["params"].cuda(), H, W), inp["K"], what="intr")
    got, want = seen_gpu(inp, chained=True), seen_reference(inp, chained=True)
    what = "seen_surface chained %s" % (crop,)
    check_seen(got, want, what)
    print("%s d_params: %.3e" % (what, relerr(got["d_leaf"], want["d_leaf"])))
    close(got["d_leaf"], want["d_leaf"], rtol=SEEN_GRAD, what=what + " d_params")


@pytest.mark.parametrize("crop", [SEEN_CROPS[0], SEEN_CROPS[3]], ids=lambda c: "%dx%d_dsp%d" % c[2:])
def test_seen_surface_backward_with_an_empty_sample(crop):
    """A sample without a valid pixel: its d_depth and d_intr are exactly zero and finite, the other sample's are what
    they are without it."""
    inp = seen_inputs(crop)
    full = seen_gpu(inp)
    emptied = inp["mask"].clone()
    emptied[0] = 0
    got = seen_gpu(inp, mask=emptied)
    for k in ("d_depth", "d_leaf"):
        assert bool(torch.isfinite(got[k]).all()), k
        assert float(got[k][0].abs().max()) == 0, k
        assert torch.equal(got[k][1], full[k][1]), k


# =====================================================================================================
# E. gradient clipping
# =====================================================================================================
CLIP_SHAPES = [(300, 70), (70,), (5, 5, 3, 3), (16384,), (16385,), (40000,), (1,)]


def clip_params(seed=2):
    g = torch.Generator().manual_seed(seed)
    return g, [torch.randn(s, generator=g) for s in CLIP_SHAPES]


def clip_grads(g):
    return [torch.randn(s, generator=g) for s in CLIP_SHAPES]


def _groups(ps):
    return [dict(params=ps[:2], lr=3e-3, weight_decay=0.0), dict(params=ps[2:], lr=1e-3, weight_decay=0.05)]


def _pair():
    """(float64 CPU parameters under torch.optim.AdamW, the same on the GPU under FusedAdamW, the generator)."""
    from zeroshape_amd.optim import FusedAdamW
    g, init = clip_params()
    ref = [p.double().requires_grad_(True) for p in init]
    mine = [p.clone().cuda().requires_grad_(True) for p in init]
    return (ref, torch.optim.AdamW(_groups(ref), betas=(0.9, 0.95)), mine, FusedAdamW(_groups(mine), betas=(0.9, 0.95)), g)


# (tensor, element) -> value: the last element of the one-chunk tensor, the one-element second chunk of (16385,) and the
# one-element tensor carry weight, so a lost tail chunk or tensor moves the norm by 1e-3 of itself
GRAD_NORM_EDGES = {(3, 16383): 30.0, (4, 16384): -20.0, (6, 0): 40.0}


def grad_norm_inputs():
    g, init = clip_params()
    grads = clip_grads(g)
    for (t, e), v in GRAD_NORM_EDGES.items():
        grads[t].view(-1)[e] = v
    return init, grads


def norm64(grads):
    return float(torch.cat([gr.double().reshape(-1) for gr in grads]).norm())


def test_grad_norm_matches_float64_and_skips_missing_gradients():
    """zs_sumsq_multi over tensors below, at and above one 16,384-element chunk, all together and each tensor alone
    under an optimiser of its own; a parameter without a gradient is skipped."""
    from zeroshape_amd.optim import FusedAdamW
    init, grads = grad_norm_inputs()
    mine = [p.clone().cuda().requires_grad_(True) for p in init + [torch.ones(123)]]
    for p, gr in zip(mine, grads):
        p.grad = gr.cuda()
    assert mine[-1].grad is None
    opt = FusedAdamW(_groups(mine), betas=(0.9, 0.95))
    want, got = norm64(grads), float(opt.grad_norm())
    print("grad_norm: %.9g (float64 %.9g), error %.2e" % (got, want, abs(got - want) / want))
    assert abs(got - want) <= GRAD_NORM_TOL * want
    for i, (p, gr) in enumerate(zip(mine, grads)):
        want, got = norm64([gr]), float(FusedAdamW([p, mine[-1]]).grad_norm())
        print("grad_norm of tensor %d %s: %.9g (float64 %.9g), error %.2e" % (i, tuple(gr.shape), got, want, abs(got - want) / want))
        assert abs(got - want) <= GRAD_NORM_TOL * want, (i, got, want)
    before = mine[-1].detach().clone()
    opt.step()
    assert torch.equal(mine[-1].detach(), before) and mine[-1] not in opt.state


# max_norm per step.  AdamW's m / sqrt(v) does not change when every gradient is scaled by the same factor, so a clip
# factor that is the same on every step barely shows in the parameters: the factors differ by up to 200 x between steps.
CLIP_BELOW = [7.5, 150.0, 30.0, 0.75]
SCALER_CLIP = [0.5, 40.0, 0.5, 3.0, 0.5]


@pytest.mark.parametrize("mode", ["below", "above", "alternate"])
def test_clip_grad_norm_then_step(mode):
    """clip_grad_norm_(max_norm) folded into the next step() against torch.nn.utils.clip_grad_norm_ + AdamW: max_norm
    below the norm (~306) on every step, a different one each step (CLIP_BELOW); above it (scale exactly 1); on steps 0
    and 2 only - the armed scale does not leak into the unclipped step behind it."""
    ref, o_ref, mine, o_mine, g = _pair()
    for step in range(4):
        max_norm = 1e4 if mode == "above" else CLIP_BELOW[step]
        grads = clip_grads(g)
        for pr, pm, gr in zip(ref, mine, grads):
            pr.grad, pm.grad = gr.double(), gr.cuda()
        if mode != "alternate" or step % 2 == 0:
            want = torch.nn.utils.clip_grad_norm_(ref, max_norm)
            got = o_mine.clip_grad_norm_(max_norm)
            assert abs(float(got) - float(want)) <= GRAD_NORM_TOL * float(want)
            assert (float(o_mine._clip) == 1.0) == (mode == "above")
        else:
            assert o_mine._clip is None
        o_ref.step()
        o_mine.step()
        o_ref.zero_grad()
        o_mine.zero_grad()
    for i, (pr, pm) in enumerate(zip(ref, mine)):
        close(pm, pr, rtol=ADAMW, what="param %d (%s)" % (i, mode))


def test_loss_scaler_step_with_clipping():
    """LossScaler.step(optim, clip_norm) on gradients pre-multiplied by the scale, clip_norm 0.5 / 40 / 3 from step to step
    (SCALER_CLIP), one overflow step among five: the parameters equal torch's clipped AdamW on the four clean steps, the
    returned norm is the unscaled one."""
    from zeroshape_amd.optim import LossScaler
    ref, o_ref, mine, o_mine, g = _pair()
    scaler = LossScaler("cuda", init_scale=1024.0)
    for step in range(5):
        overflow = step == 2
        scale = float(scaler.scale)
        grads = clip_grads(g)
        for pr, pm, gr in zip(ref, mine, grads):
            pm.grad = gr.cuda() * scale
            if overflow:
                pm.grad.view(-1)[0] = float("inf")
            else:
                pr.grad = gr.double()
        got = scaler.step(o_mine, clip_norm=SCALER_CLIP[step])
        if overflow:
            assert not bool(torch.isfinite(got))
        else:
            want = torch.nn.utils.clip_grad_norm_(ref, SCALER_CLIP[step])
            assert abs(float(got) - float(want)) <= GRAD_NORM_TOL * float(want), (step, float(got), float(want))
            o_ref.step()
        o_ref.zero_grad()
        o_mine.zero_grad()
    assert float(scaler.scale) == 512.0
    for i, (pr, pm) in enumerate(zip(ref, mine)):
        close(pm, pr, rtol=ADAMW, what="param %d" % i)
    assert o_mine.state_dict()["state"][0]["step"] == 4
