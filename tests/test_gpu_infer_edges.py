"""GPU parity of the inference layer kernels (csrc/nn_ops.hip, the resampling kernels of csrc/nn_train_norm.hip and
zs_transform_points) on every branch their launchers take and at the shapes where an indexing slip shows: channel counts
that are no multiple of 4 or of 64, one row / one pixel, maps smaller than a window, slices on both sides of the GroupNorm
cache gate, sequence lengths on both sides of every attention gate.  tests/test_gpu_nn_layers.py runs most of these ops
at one or two shapes; the branches named in the comments below are launched by no other test.

Reference: torch on the CPU in float64, on the same fp32 input values upcast - torch.nn.functional where it states the op,
plain tensor ops where it does not (tests/test_infer_edge_refs.py pins the plain ones against the functional forms).
Comparison: the `close` the existing test of the same op uses, at that test's tolerance; the constants marked "measured"
are max(that tolerance, 4 x the error of fp32 CPU torch against the float64 reference on the same input), and
tests/test_infer_edge_refs.py recomputes that noise on the CPU and pins them.  The same module maps every case below to
the kernel the launcher sends it to and asserts that no reachable kernel is left without a case.

The builders / references below run on the CPU alone (the CPU module imports them)."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_nn_layers import close, same_pad
from tests.test_gpu_train_edges import group_norm_two_pass, relerr
from tests.test_gpu_train_ops import close as close_adjoint

pytestmark = pytest.mark.gpu

F64 = torch.float64

NORM, ATTENTION = 2e-5, 2e-5                   # of the output scale (test_layer_norm, test_group_norm, test_attention)
UPSAMPLE, GLOBAL_MEAN = 2e-6, 1e-6             # test_pooling_and_resampling
ADJOINT = 2e-5                                 # test_upsample_global_mean_layout_and_token_adjoints (resize_grid too)

# ---- measured constants: max(table value, 4 x fp32-CPU-torch error against float64 on the same input) ----
# x = 64 + 0.5 randn through F.layer_norm in fp32: 5.43e-6 of scale at 150 x 384, 6.83e-6 at 150 x 770
#   -> 4 x 5.43e-6 = 2.17e-5 and 4 x 6.83e-6 = 2.73e-5, both above the table's 2e-5.
LN_ILL_TOL = {(150, 384): 2.2e-5, (150, 770): 2.8e-5}
# x = 64 + 0.5 randn through group_norm_two_pass in fp32 at 2 x 120 x 120 x 8, 4 groups (28,800 values of ~64 per fp32
# mean): 4.70e-5 of scale -> 4 x 4.70e-5 = 1.88e-4, above the table's 2e-5.  (F.group_norm in fp32, with its one-pass
# variance, is off by 3.8e-3 there.)
GN_ILL_TOL = 1.9e-4
# qkv x 4 at (16, 225, 8, 32): fp32 torch 3.57e-6 of scale -> 4 x 3.57e-6 = 1.43e-5, below the table: the table holds.
ATT_BIG_TOL = ATTENTION
# transform_points (it had no op-level tolerance): fp32 torch ((p @ R^T + t) - mean) / scale against float64, the worst of
# the ten (B, n) cases: 2.36e-7 of scale with the mean near the translation -> 4 x 2.36e-7 = 9.43e-7; 7.60e-8 with zero
# mean and unit scale -> 4 x 7.60e-8 = 3.04e-7.
TRANSFORM_TOL, TRANSFORM_EVAL_TOL = 9.5e-7, 3.1e-7


def check(got, want, tol, what):
    print("%s: %.3e (tolerance %.1e)" % (what, relerr(got, want), tol))
    close(got, want, tol)


def check_adjoint(got, want, tol, what):
    print("%s: %.3e (tolerance %.1e)" % (what, relerr(got, want), tol))
    close_adjoint(got, want, rtol=tol, what=what)


def bit_equal(got, want, what):
    """tol = 0, infinities included (`close` subtracts, and -inf - -inf is no number)."""
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    print("%s: %d of %d elements differ (tolerance 0)" % (what, int((got != want).sum()), want.numel()))
    if bool(torch.isfinite(want).all()):
        close(got, want, 0)
    assert torch.equal(got, want), what


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


# =====================================================================================================
# A. LayerNorm: zs_layer_norm, four rows (one wave each) per workgroup
# =====================================================================================================
LN_ROWS = [1, 3, 4, 5, 150]                    # a quarter-filled workgroup, one short of / exactly / one over a full one, 38 of them
LN_C = [
    4,       # layer_norm_reg_kernel<1> (C % 4 == 0, C <= 256): one quad, lanes 1..63 hold nothing
    252,     # <1>: 63 quads, lane 63 idle
    256,     # <1>: every lane one quad - the last C of <1>
    260,     # layer_norm_reg_kernel<2> (256 < C <= 512): the second vector holds one quad, in lane 0
    384,     # <2>: the second vector half full
    512,     # <2>: both vectors full - the last C of <2>
    516,     # layer_norm_reg_kernel<4> (512 < C <= 1024): one quad in the third vector
    1024,    # <4>: all four vectors full - the last C of <4>
    1028,    # layer_norm_kernel (C > 1024): the scalar kernel on a multiple of 4
    1536,    # layer_norm_kernel: 24 elements per lane
    1,       # layer_norm_kernel (C % 4 != 0): zero variance, y = beta
    7,       # layer_norm_kernel: fewer elements than lanes
    97,      # layer_norm_kernel: a ragged second sweep
    770,     # layer_norm_kernel: C % 4 == 2 beside the ViT's 768
]
LN_ILL_CASES = [(150, 384), (150, 770)]        # layer_norm_reg_kernel<2>, layer_norm_kernel


def ln_inputs(rows, C, ill=False):
    g = _gen(1, rows, C)
    x = torch.randn(rows, C, generator=g)
    return dict(x=64 + 0.5 * x if ill else x * 2 + 0.5, gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g))


def ln_reference(inp, dtype=F64):
    return F.layer_norm(inp["x"].to(dtype), (inp["x"].shape[-1],), inp["gamma"].to(dtype), inp["beta"].to(dtype), 1e-6)


def ln_gpu(inp):
    from zeroshape_amd.nn import ops
    return ops.layer_norm(inp["x"].cuda(), inp["gamma"].cuda(), inp["beta"].cuda(), 1e-6)


@pytest.mark.parametrize("C", LN_C)
def test_layer_norm_every_kernel_and_row_count(C):
    for rows in LN_ROWS:
        inp = ln_inputs(rows, C)
        want = ln_reference(inp)
        if C == 1:
            assert torch.equal(want, inp["beta"].double().expand(rows, 1))
        check(ln_gpu(inp), want, NORM, "layer_norm %dx%d" % (rows, C))


@pytest.mark.parametrize("rows,C", LN_ILL_CASES)
def test_layer_norm_ill_conditioned(rows, C):
    """x = 64 + 0.5 randn: mean^2 is 16,000 x the variance; the kernels take the variance about the mean."""
    inp = ln_inputs(rows, C, ill=True)
    check(ln_gpu(inp), ln_reference(inp), LN_ILL_TOL[(rows, C)], "layer_norm ill %dx%d" % (rows, C))


# =====================================================================================================
# B. GroupNorm: zs_group_norm_nhwc (every tensor below 8 MiB: ops.group_norm passes no workspace, one launch)
# =====================================================================================================
# (B, H, W, C, groups, relu, residual)
GN_CASES = [
    # group_norm_kernel: C / groups = 3, 6, 5 is no power of two; 63 pixels, 189 / 378 / 315 elements per slice
    (2, 7, 9, 96, 32, True, False),
    (2, 7, 9, 12, 2, False, True),
    (2, 7, 9, 10, 2, True, True),
    # group_norm_pow2_kernel<VEC, CACHE>: VEC = min(4, C / groups); CACHE = the slice (H W C / groups floats) fits GN_CACHE_BYTES
    # = 114,688 bytes.  Each width at the smallest square map above the gate and at the one below it.
    (2, 170, 170, 4, 4, False, False),       # <1, false>: 28,900 floats = 115,600 bytes
    (2, 169, 169, 4, 4, True, True),         # <1, true>: 114,244 bytes
    (2, 120, 120, 8, 4, True, False),        # <2, false>: 115,200 bytes
    (2, 119, 119, 8, 4, False, True),        # <2, true>: 113,288 bytes
    (2, 85, 85, 16, 4, False, True),         # <4, false>, one vector per pixel (shift 0): 115,600 bytes
    (2, 84, 84, 16, 4, True, False),         # <4, true>: 112,896 bytes
    (2, 43, 43, 64, 4, True, True),          # <4, false>, four vectors per pixel (shift 2): 118,336 bytes
    (2, 42, 42, 64, 4, False, False),        # <4, true>: 112,896 bytes
]
GN_ILL_CASE = (2, 120, 120, 8, 4, False, True)     # group_norm_pow2_kernel<2, false>
GN_TWO_LAUNCH_BYTES = 8 << 20                  # ops.group_norm hands a workspace from here on


def gn_inputs(cfg, ill=False):
    B, H, W, C, groups, relu, res = cfg
    g = _gen(2, H, W, C, groups)
    x = torch.randn(B, H, W, C, generator=g)                       # channels-last
    return dict(x=64 + 0.5 * x if ill else x * 3 + 1, gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g),
                res=torch.randn(B, H, W, C, generator=g) if res else None, groups=groups, relu=relu)


def gn_reference(inp, dtype=F64, two_pass=False):
    x, ga, be = inp["x"].to(dtype), inp["gamma"].to(dtype), inp["beta"].to(dtype)
    if two_pass:
        y = group_norm_two_pass(x, inp["groups"], ga, be, 1e-5)
    else:
        y = F.group_norm(x.permute(0, 3, 1, 2), inp["groups"], ga, be, 1e-5).permute(0, 2, 3, 1)
    if inp["res"] is not None:
        y = y + inp["res"].to(dtype)
    return F.relu(y) if inp["relu"] else y


def gn_gpu(inp):
    from zeroshape_amd.nn import ops
    assert inp["x"].numel() * 4 < GN_TWO_LAUNCH_BYTES
    return ops.group_norm(inp["x"].cuda(), inp["gamma"].cuda(), inp["beta"].cuda(), inp["groups"], 1e-5, inp["relu"],
                          None if inp["res"] is None else inp["res"].cuda())


@pytest.mark.parametrize("cfg", GN_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_group_norm_generic_and_both_sides_of_the_cache_gate(cfg):
    inp = gn_inputs(cfg)
    check(gn_gpu(inp), gn_reference(inp), NORM, "group_norm %s" % (cfg,))


def test_group_norm_ill_conditioned_uncached():
    """x = 64 + 0.5 randn re-read from memory for the output pass; the reference takes the variance about the mean."""
    inp = gn_inputs(GN_ILL_CASE, ill=True)
    check(gn_gpu(inp), gn_reference(inp, two_pass=True), GN_ILL_TOL, "group_norm ill %s" % (GN_ILL_CASE,))


# =====================================================================================================
# C. max pool: zs_max_pool_nhwc
# =====================================================================================================
POOL_C = [
    1, 3, 5, 6,      # max_pool_kernel (C % 4 != 0): one channel, odd counts, C % 4 == 2
    64,              # max_pool_quad_kernel (C % 4 == 0) on the same windows
]
POOL_WINDOWS = [(3, 2, 1), (3, 2, "same"), (2, 2, 0), (3, 1, 1)]       # (k, stride, padding)
POOL_MAPS = [(1, 1), (2, 5), (17, 20)]         # smaller than a window; 1 or 2 output rows; several 256-lane blocks
POOL_KINDS = ["relu", "inf"]


def pool_input(C, H, W, kind):
    """Post-ReLU values (half of them 0: ties in most windows) or randn with four in ten entries and the top left corner of
    sample 0 at -inf."""
    g = _gen(3, C, H, W)
    x = torch.randn(2, H, W, C, generator=g)
    if kind == "relu":
        return F.relu(x)
    x = torch.where(torch.rand(2, H, W, C, generator=g) < 0.4, torch.full_like(x, float("-inf")), x)
    x[0, :4, :4] = float("-inf")                                   # the first window of sample 0 holds nothing else
    return x


def pool_out_size(n, k, stride, padding):
    return -(-n // stride) if padding == "same" else (n + 2 * padding - k) // stride + 1


def pool_reference(x, k, stride, padding, dtype=F64):
    x = x.to(dtype).permute(0, 3, 1, 2)
    if padding == "same":
        x, padding = same_pad(x, k, stride, value=float("-inf")), 0
    return F.max_pool2d(x, k, stride, padding).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("C", POOL_C)
def test_max_pool_scalar_and_quad_kernels(C):
    from zeroshape_amd import _lib
    from zeroshape_amd.nn import ops
    for H, W in POOL_MAPS:
        for k, stride, padding in POOL_WINDOWS:
            for kind in POOL_KINDS:
                x = pool_input(C, H, W, kind)
                what = "max_pool C=%d %dx%d k=%d s=%d p=%s %s" % (C, H, W, k, stride, padding, kind)
                if min(pool_out_size(H, k, stride, padding), pool_out_size(W, k, stride, padding)) < 1:
                    with pytest.raises(RuntimeError):              # no output pixel (2 x 2 window on the 1 x 1 map): torch
                        pool_reference(x, k, stride, padding)      # refuses it, and so does the launcher
                    with pytest.raises(_lib.ZeroShapeHipError):
                        ops.max_pool(x.cuda(), k, stride, padding)
                    continue
                bit_equal(ops.max_pool(x.cuda(), k, stride, padding), pool_reference(x, k, stride, padding), what)


# =====================================================================================================
# D. global mean: zs_global_mean_nhwc, 64 channels x 4 pixel slices per workgroup
# =====================================================================================================
MEAN_C = [1, 63, 64, 65, 100, 130]             # one lane; a ragged / full block; a second block of 1 / 36; a third of 2
MEAN_MAPS = [(1, 1), (1, 2), (3, 1), (1, 5), (7, 7)]   # HW = 1, 2, 3: empty slices; 5: one slice twice; 49
MEAN_B = [1, 3]


def mean_input(B, H, W, C):
    return torch.randn(B, H, W, C, generator=_gen(4, B, H, W, C)) + 0.5


def mean_reference(x, dtype=F64):
    return x.to(dtype).mean((1, 2))


@pytest.mark.parametrize("C", MEAN_C)
def test_global_mean_ragged_blocks_and_empty_slices(C):
    from zeroshape_amd.nn import ops
    for B in MEAN_B:
        for H, W in MEAN_MAPS:
            x = mean_input(B, H, W, C)
            check(ops.global_mean(x.cuda()), mean_reference(x), GLOBAL_MEAN, "global_mean %dx%dx%dx%d" % (B, H, W, C))


# =====================================================================================================
# E. x2 bilinear (align_corners) and its adjoint: zs_upsample2x_nhwc, zs_upsample2x_bwd_nhwc
# =====================================================================================================
UP_MAPS = [(1, 1), (2, 2), (2, 7), (3, 2), (5, 1)]     # Hin = 2: the adjoint's window [2 iy - 3, 2 iy + 4] covers every output row
UP_C = [
    1, 3,    # upsample2x_kernel, upsample2x_bwd_kernel<1> (C % 4 != 0)
    4, 8,    # upsample2x_vec_kernel, upsample2x_bwd_kernel<4> (C % 4 == 0): one / two quads per pixel
]


def up_inputs(H, W, C):
    g = _gen(5, H, W, C)
    return dict(x=torch.randn(2, H, W, C, generator=g), gy=torch.randn(2, 2 * H, 2 * W, C, generator=g))


def up_reference(inp, dtype=F64):
    x = inp["x"].detach().to(dtype).clone().requires_grad_(True)
    y = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    y.backward(inp["gy"].to(dtype))
    return dict(forward=y.detach(), dx=x.grad)


@pytest.mark.parametrize("C", UP_C)
def test_upsample2x_small_maps_forward_and_backward(C):
    from zeroshape_amd.nn import autograd as A
    for H, W in UP_MAPS:
        inp = up_inputs(H, W, C)
        want = up_reference(inp)
        x = inp["x"].cuda().requires_grad_(True)
        y = A.upsample2x(x)
        y.backward(inp["gy"].cuda())
        check(y, want["forward"], UPSAMPLE, "upsample2x %dx%dx%d forward" % (H, W, C))
        check_adjoint(x.grad, want["dx"], ADJOINT, "upsample2x %dx%dx%d backward" % (H, W, C))


# =====================================================================================================
# F. position-grid resize (align_corners=False) and its adjoint: zs_resize_bilinear_nhwc
# =====================================================================================================
# (Hi, Wi, Ho, Wo): shrinking to a non-square grid, enlarging one side and shrinking the other, the identity, everything into
# one pixel, x2, and one pixel spread over nine
RESIZE_CASES = [(24, 24, 9, 20), (24, 24, 30, 17), (24, 24, 24, 24), (24, 24, 1, 1), (24, 24, 48, 48), (1, 1, 3, 3)]
RESIZE_C = [1, 32]


def resize_inputs(Hi, Wi, Ho, Wo, C):
    g = _gen(6, Hi, Ho, Wo, C)
    return dict(x=torch.randn(Hi, Wi, C, generator=g), gy=torch.randn(Ho, Wo, C, generator=g))


def resize_reference(inp, dtype=F64):
    x = inp["x"].detach().to(dtype).clone().requires_grad_(True)
    Ho, Wo = inp["gy"].shape[:2]
    y = F.interpolate(x.permute(2, 0, 1)[None], size=(Ho, Wo), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    y.backward(inp["gy"].to(dtype))
    return dict(forward=y.detach(), dx=x.grad)


@pytest.mark.parametrize("C", RESIZE_C)
@pytest.mark.parametrize("Hi,Wi,Ho,Wo", RESIZE_CASES)
def test_resize_grid_non_square_and_enlarging(Hi, Wi, Ho, Wo, C):
    from zeroshape_amd.nn import autograd as A
    inp = resize_inputs(Hi, Wi, Ho, Wo, C)
    want = resize_reference(inp)
    if (Hi, Wi) == (Ho, Wo):
        assert torch.equal(want["forward"], inp["x"].double())
    x = inp["x"].cuda().requires_grad_(True)
    y = A.resize_grid(x, Ho, Wo)
    y.backward(inp["gy"].cuda())
    what = "resize_grid %dx%d->%dx%d C=%d" % (Hi, Wi, Ho, Wo, C)
    check_adjoint(y, want["forward"], ADJOINT, what + " forward")
    check_adjoint(x.grad, want["dx"], ADJOINT, what + " backward")


# =====================================================================================================
# G. layout and tokens: zs_nchw_to_nhwc, zs_nhwc_to_nchw, zs_assemble_tokens, zs_readout_concat
# =====================================================================================================
LAYOUT_C = [1, 3, 5]
LAYOUT_CPAD = [None, 4, 8]
LAYOUT_MAPS = [(1, 1), (7, 9)]
NCHW_C = [1, 5]
TOKEN_CASES = [(1, 1, 1), (3, 5, 7), (2, 196, 768)]    # (B, n, C)


def layout_inputs(C, H, W):
    g = _gen(7, C, H, W)
    return dict(x=torch.randn(2, C, H, W, generator=g), mask=(torch.rand(2, 1, H, W, generator=g) > 0.4).float())


def to_nhwc_reference(inp, cpad, masked, dtype=F64):
    x = inp["x"].to(dtype)
    if masked:
        x = x * inp["mask"].to(dtype)
    return F.pad(x.permute(0, 2, 3, 1), (0, (cpad or x.shape[1]) - x.shape[1])).contiguous()


@pytest.mark.parametrize("C", LAYOUT_C)
def test_to_nhwc_padding_and_mask(C):
    from zeroshape_amd import _lib
    from zeroshape_amd.nn import ops
    for H, W in LAYOUT_MAPS:
        inp = layout_inputs(C, H, W)
        for cpad in LAYOUT_CPAD:
            for masked in (False, True):
                mask = inp["mask"].cuda() if masked else None
                if cpad is not None and cpad < C:                      # 5 channels into 4: refused, nothing cut off
                    with pytest.raises(_lib.ZeroShapeHipError):
                        ops.to_nhwc(inp["x"].cuda(), cpad=cpad, mask=mask)
                    continue
                bit_equal(ops.to_nhwc(inp["x"].cuda(), cpad=cpad, mask=mask), to_nhwc_reference(inp, cpad, masked),
                          "to_nhwc C=%d %dx%d cpad=%s mask=%s" % (C, H, W, cpad, masked))


@pytest.mark.parametrize("C", NCHW_C)
def test_to_nchw(C):
    from zeroshape_amd.nn import ops
    for H, W in LAYOUT_MAPS:
        x = torch.randn(2, H, W, C, generator=_gen(8, C, H, W))
        bit_equal(ops.to_nchw(x.cuda()), x.double().permute(0, 3, 1, 2), "to_nchw C=%d %dx%d" % (C, H, W))


def token_inputs(B, n, C):
    """Multiples of 2^-10 below 4: every cls + pos and feat + pos is exact in fp32, so the float64 reference and the
    kernel's fp32 sum are the same number."""
    g = _gen(9, B, n, C)
    q = lambda *shape: torch.randint(-4095, 4096, shape, generator=g).float() / 1024       # noqa: E731
    return dict(feat=q(B, n, C), cls=q(C), pos=q(n + 1, C))


def token_reference(inp, dtype=F64):
    feat, cls, pos = [inp[k].to(dtype) for k in ("feat", "cls", "pos")]
    B, n, C = feat.shape
    tok = torch.cat([cls.expand(B, 1, C), feat], 1) + pos
    return dict(tokens=tok, readout=torch.cat([tok[:, 1:], tok[:, :1].expand(-1, n, -1)], -1))


@pytest.mark.parametrize("B,n,C", TOKEN_CASES)
def test_assemble_tokens_then_readout_concat(B, n, C):
    from zeroshape_amd.nn import ops
    inp = token_inputs(B, n, C)
    want = token_reference(inp)
    tok = ops.assemble_tokens(inp["feat"].cuda(), inp["cls"].cuda(), inp["pos"].cuda())
    bit_equal(tok, want["tokens"], "assemble_tokens %s" % ((B, n, C),))
    bit_equal(ops.readout_concat(tok), want["readout"], "readout_concat %s" % ((B, n, C),))


# =====================================================================================================
# H. attention: zs_attention (CONV_PRECISION "f32") and zs_attention_split ("f16x3")
# =====================================================================================================
# (B, L, heads, d).  Under "f32" every case runs attention_kernel<d>; the comments name the kernel under "f16x3".
ATT_CASES = [
    # 4 (sample, head) pairs, at most two key tiles: 4 x tiles < 512 but L <= 64, fewer than 128 pairs -> attention_split_kernel<d>
    (2, 1, 2, 32), (2, 31, 2, 32), (2, 32, 2, 32), (2, 33, 2, 32), (2, 64, 2, 32),      # one key, a ragged tile, one tile,
    (2, 1, 2, 64), (2, 31, 2, 64), (2, 32, 2, 64), (2, 33, 2, 64), (2, 64, 2, 64),      # one key beyond it, two full tiles
    # 128 pairs, d = 32
    (16, 32, 8, 32),     # L > 32 fails -> attention_split_kernel<32>
    (16, 33, 8, 32),     # 128 x 2 < 512 but L <= 64; >= 128 pairs and 32 < L <= 96 -> attention_lds_kernel<32, 96>
    (16, 96, 8, 32),     # 128 x 3 < 512 and L > 64 -> attention_split_kw_kernel<32> (the key-split form takes it first)
    (16, 97, 8, 32),     # 128 x 4 = 512 -> attention_lds_kernel<32, 224>
    (16, 224, 8, 32),    # the last L of attention_lds_kernel<32, 224>
    (16, 225, 8, 32),    # L <= 224 fails -> attention_split_kernel<32>, eight key tiles
    # the d = 64 forms of the three gated kernels, which the sizes above leave out
    (2, 97, 2, 64),      # 4 x 4 < 512 and L > 64 -> attention_split_kw_kernel<64>
    (16, 33, 8, 64),     # attention_lds_kernel<64, 96>
    (16, 97, 8, 64),     # attention_lds_kernel<64, 224>
]
ATT_BIG_CASE = (16, 225, 8, 32)                # qkv x 4: logits of +-40 over eight key tiles
ATT_PRECISIONS = ["f32", "f16x3"]


def attention_inputs(B, L, heads, d, mult=1.0):
    return dict(qkv=torch.randn(B, L, 3 * heads * d, generator=_gen(10, B, L, heads, d)) * mult, heads=heads)


def attention_reference(inp, dtype=F64):
    qkv = inp["qkv"].to(dtype)
    B, L, C3 = qkv.shape
    heads = inp["heads"]
    d = C3 // 3 // heads
    q, k, v = qkv.reshape(B, L, 3, heads, d).permute(2, 0, 3, 1, 4).unbind(0)
    return (((q @ k.transpose(-2, -1)) * d ** -0.5).softmax(-1) @ v).transpose(1, 2).reshape(B, L, heads * d)


def attention_gpu_both(inp, want, tol, what, monkeypatch):
    from zeroshape_amd.nn import ops
    qkv = inp["qkv"].cuda()
    for prec in ATT_PRECISIONS:
        monkeypatch.setattr(ops, "CONV_PRECISION", prec)
        check(ops.attention(qkv, inp["heads"]), want, tol, "attention %s %s" % (what, prec))


@pytest.mark.parametrize("B,L,heads,d", ATT_CASES)
def test_attention_on_both_sides_of_every_gate(B, L, heads, d, monkeypatch):
    inp = attention_inputs(B, L, heads, d)
    attention_gpu_both(inp, attention_reference(inp), ATTENTION, str((B, L, heads, d)), monkeypatch)


def test_attention_large_logits_over_eight_key_tiles(monkeypatch):
    inp = attention_inputs(*ATT_BIG_CASE, mult=4.0)
    attention_gpu_both(inp, attention_reference(inp), ATT_BIG_TOL, "x4 %s" % (ATT_BIG_CASE,), monkeypatch)


# =====================================================================================================
# I. camera.transform_points: zs_transform_points, 256 points per workgroup
# =====================================================================================================
TP_B = [1, 3]
TP_N = [1, 255, 256, 257, 1000]                # one point; one short of / exactly / one over a workgroup; four workgroups


def tp_inputs(B, n, evaluation=False):
    """A random orthonormal rotation, a translation of length 2, points in the unit cube about the origin; the mean within
    0.05 of the translation (cam - mean cancels) and a scale in [0.3, 2] - or, evaluation, zero mean and unit scale."""
    g = _gen(11, B, n)
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    t = torch.randn(B, 3, generator=g)
    t = 2 * t / t.norm(dim=1, keepdim=True)
    mean, scale = t + 0.05 * torch.randn(B, 3, generator=g), 0.3 + 1.7 * torch.rand(B, generator=g)
    if evaluation:
        mean, scale = torch.zeros(B, 3), torch.ones(B)
    return dict(points=torch.rand(B, n, 3, generator=g) - 0.5, pose=torch.cat([R, t[..., None]], -1), mean=mean, scale=scale)


def tp_reference(inp, dtype=F64):
    p, T, m, s = [inp[k].to(dtype) for k in ("points", "pose", "mean", "scale")]
    cam = p @ T[:, :, :3].transpose(1, 2) + T[:, None, :, 3]
    return (cam - m[:, None]) / s[:, None, None]


@pytest.mark.parametrize("evaluation", [False, True], ids=["training", "evaluation"])
def test_transform_points(evaluation):
    from zeroshape_amd.utils import camera
    for B in TP_B:
        for n in TP_N:
            inp = tp_inputs(B, n, evaluation)
            got = camera.transform_points(*[inp[k].cuda() for k in ("points", "pose", "mean", "scale")])
            check(got, tp_reference(inp), TRANSFORM_EVAL_TOL if evaluation else TRANSFORM_TOL, "transform_points B=%d n=%d%s" % (B, n, " eval" if evaluation else ""))


def test_transform_points_refuses_cpu_tensors():
    from zeroshape_amd.utils import camera
    inp = tp_inputs(1, 5)
    for on_cpu in ("points", "pose", "mean", "scale"):
        args = [inp[k] if k == on_cpu else inp[k].cuda() for k in ("points", "pose", "mean", "scale")]
        with pytest.raises(ValueError):
            camera.transform_points(*args)
