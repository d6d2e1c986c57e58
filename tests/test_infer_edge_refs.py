"""CPU side of tests/test_gpu_infer_edges.py: the evidence that its references, tolerances and cases are sound.

 - noise: every "measured" tolerance of the GPU module is at least 4 x the error of fp32 CPU torch against the float64
   reference on the same input, recomputed here; every table tolerance is at least 4 x that error on the cases it is used
   for; every bit-equal demand holds between fp32 and float64 torch on those inputs;
 - references: every reference written in plain tensor ops agrees with the torch.nn.functional form in float64 to 1e-9
   where both exist;
 - branch accounting: a restatement of the launcher conditions of zs_layer_norm, zs_group_norm_nhwc, zs_max_pool_nhwc,
   zs_upsample2x_nhwc, zs_upsample2x_bwd_nhwc, zs_attention_split and zs_attention, with its thresholds read from the
   source text, maps each case of the GPU module to a kernel; every kernel those launchers name must have a case, and
   the cases must sit on both sides of every threshold."""
import collections
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import test_gpu_infer_edges as E
from tests.test_gpu_train_ops import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32


def noise(ref_fn, *args, **kw):
    """fp32 CPU torch against float64, as `close` measures it; dicts (forward, dx) give their worst entry."""
    lo, hi = ref_fn(*args, dtype=F32, **kw), ref_fn(*args, dtype=E.F64, **kw)
    if isinstance(hi, dict):
        return max(E.relerr(lo[k], hi[k]) for k in hi)
    return E.relerr(lo, hi)


def covered(what, err, tol):
    print("%s: fp32 torch against float64 %.2e, tolerance %.1e" % (what, err, tol))
    assert 4 * err <= tol, "%s: 4 x %.3e above the tolerance %.3e" % (what, err, tol)


# =====================================================================================================
# noise
# =====================================================================================================
def test_measured_tolerances_cover_fp32_noise():
    for c in E.LN_ILL_CASES:
        covered("layer_norm ill %s" % (c,), noise(E.ln_reference, E.ln_inputs(*c, ill=True)), E.LN_ILL_TOL[c])
        assert E.LN_ILL_TOL[c] >= E.NORM
    covered("group_norm ill", noise(E.gn_reference, E.gn_inputs(E.GN_ILL_CASE, ill=True), two_pass=True), E.GN_ILL_TOL)
    covered("attention x4", noise(E.attention_reference, E.attention_inputs(*E.ATT_BIG_CASE, mult=4.0)), E.ATT_BIG_TOL)
    assert E.GN_ILL_TOL >= E.NORM and E.ATT_BIG_TOL >= E.ATTENTION
    for evaluation, tol in ((False, E.TRANSFORM_TOL), (True, E.TRANSFORM_EVAL_TOL)):
        worst = max(noise(E.tp_reference, E.tp_inputs(B, n, evaluation)) for B in E.TP_B for n in E.TP_N)
        covered("transform_points%s" % (" evaluation" if evaluation else ""), worst, tol)
        assert tol <= 5 * worst                                     # the rule's value: no table value stands behind it
        assert tol <= 8 * 2.0 ** -23                                # and a few ulp of the output scale at the most


def test_table_tolerances_cover_fp32_noise():
    """The tolerances taken over from the existing tests are no tighter than 4 x what fp32 torch itself achieves on the
    new inputs (LayerNorm and GroupNorm in fp32 by the two-pass forms: F.group_norm's one-pass variance is another matter)."""
    worst = collections.defaultdict(float)
    for C in E.LN_C:
        for rows in E.LN_ROWS:
            worst["layer_norm"] = max(worst["layer_norm"], noise(E.ln_reference, E.ln_inputs(rows, C)))
    for cfg in E.GN_CASES:
        inp = E.gn_inputs(cfg)
        worst["group_norm"] = max(worst["group_norm"], E.relerr(E.gn_reference(inp, F32, two_pass=True), E.gn_reference(inp)))
    for C in E.MEAN_C:
        for B in E.MEAN_B:
            for H, W in E.MEAN_MAPS:
                worst["global_mean"] = max(worst["global_mean"], noise(E.mean_reference, E.mean_input(B, H, W, C)))
    for C in E.UP_C:
        for H, W in E.UP_MAPS:
            lo, hi = E.up_reference(E.up_inputs(H, W, C), F32), E.up_reference(E.up_inputs(H, W, C))
            worst["upsample2x"] = max(worst["upsample2x"], E.relerr(lo["forward"], hi["forward"]))
            worst["upsample2x backward"] = max(worst["upsample2x backward"], E.relerr(lo["dx"], hi["dx"]))
    for C in E.RESIZE_C:
        for c in E.RESIZE_CASES:
            worst["resize_grid"] = max(worst["resize_grid"], noise(E.resize_reference, E.resize_inputs(*c, C)))
    for c in E.ATT_CASES:
        worst["attention"] = max(worst["attention"], noise(E.attention_reference, E.attention_inputs(*c)))
    table = {"layer_norm": E.NORM, "group_norm": E.NORM, "global_mean": E.GLOBAL_MEAN, "upsample2x": E.UPSAMPLE,
             "upsample2x backward": E.ADJOINT, "resize_grid": E.ADJOINT, "attention": E.ATTENTION}
    assert sorted(table) == sorted(worst)
    for k in sorted(table):
        covered(k, worst[k], table[k])


def test_bit_equal_demands_hold_between_fp32_and_float64_torch():
    for C in E.POOL_C:
        for H, W in E.POOL_MAPS:
            for k, stride, padding in E.POOL_WINDOWS:
                for kind in E.POOL_KINDS:
                    x = E.pool_input(C, H, W, kind)
                    if min(E.pool_out_size(H, k, stride, padding), E.pool_out_size(W, k, stride, padding)) < 1:
                        assert (H, W, k) == (1, 1, 2)               # the one window that has no output pixel
                        with pytest.raises(RuntimeError):
                            E.pool_reference(x, k, stride, padding)
                        continue
                    want = E.pool_reference(x, k, stride, padding)
                    assert torch.equal(E.pool_reference(x, k, stride, padding, dtype=F32).double(), want)
                    assert want.shape[1:3] == (E.pool_out_size(H, k, stride, padding), E.pool_out_size(W, k, stride, padding))
                    if kind == "relu" and H * W > 1:                # ties: the maximum is taken more than once somewhere
                        assert float((x == 0).float().mean()) > 0.3
                    if kind == "inf":                               # windows of nothing but -inf, and finite ones
                        assert bool(torch.isinf(x).any())
                        assert bool(torch.isinf(want[0, 0, 0]).all())
                        if (H, W) == (17, 20):
                            assert bool(torch.isfinite(want).any())
    for C in E.LAYOUT_C:
        for H, W in E.LAYOUT_MAPS:
            inp = E.layout_inputs(C, H, W)
            assert set(inp["mask"].unique().tolist()) <= {0.0, 1.0}
            for cpad in E.LAYOUT_CPAD:
                if cpad is not None and cpad < C:
                    continue
                for masked in (False, True):
                    want = E.to_nhwc_reference(inp, cpad, masked)
                    assert torch.equal(E.to_nhwc_reference(inp, cpad, masked, dtype=F32).double(), want)
                    assert want.shape == (2, H, W, cpad or C) and float(want[..., C:].abs().sum()) == 0
    for c in E.TOKEN_CASES:
        inp = E.token_inputs(*c)
        lo, hi = E.token_reference(inp, dtype=F32), E.token_reference(inp)
        assert torch.equal(lo["tokens"].double(), hi["tokens"]) and torch.equal(lo["readout"].double(), hi["readout"])


# =====================================================================================================
# references
# =====================================================================================================
def test_plain_references_agree_with_the_functional_forms():
    for c in E.ATT_CASES:
        inp = E.attention_inputs(*c)
        B, L, heads, d = c
        q, k, v = inp["qkv"].double().reshape(B, L, 3, heads, d).permute(2, 0, 3, 1, 4).unbind(0)
        want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, heads * d)
        close(E.attention_reference(inp), want, rtol=1e-9, what="attention %s" % (c,))
    inp = E.attention_inputs(*E.ATT_BIG_CASE, mult=4.0)
    B, L, heads, d = E.ATT_BIG_CASE
    q, k, v = inp["qkv"].double().reshape(B, L, 3, heads, d).permute(2, 0, 3, 1, 4).unbind(0)
    close(E.attention_reference(inp), F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, heads * d),
          rtol=1e-9, what="attention x4")
    for cfg in E.GN_CASES + [E.GN_ILL_CASE]:                        # group_norm_two_pass is F.group_norm in float64
        inp = E.gn_inputs(cfg, ill=cfg == E.GN_ILL_CASE)
        close(E.gn_reference(inp, two_pass=True), E.gn_reference(inp), rtol=1e-9, what="group_norm %s" % (cfg,))
    for C in E.MEAN_C:
        for H, W in E.MEAN_MAPS:
            x = E.mean_input(3, H, W, C)
            want = F.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), 1)[:, :, 0, 0]
            close(E.mean_reference(x), want, rtol=1e-9, what="global_mean")
    for C in E.LAYOUT_C:                                            # to_nhwc without padding and mask is a permutation
        inp = E.layout_inputs(C, 7, 9)
        assert torch.equal(E.to_nhwc_reference(inp, None, False), inp["x"].double().permute(0, 2, 3, 1))
    for B in E.TP_B:                                                # transform_points: the batched GEMM it replaced
        inp = E.tp_inputs(B, 257)
        R, t = inp["pose"].double()[:, :, :3], inp["pose"].double()[:, :, 3:]
        assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=E.F64)).abs().max()) < 1e-5       # orthonormal
        assert float((t.norm(dim=1) - 2).abs().max()) < 1e-5 and float((inp["mean"] - t[..., 0]).abs().max()) < 0.3
        assert 0.3 <= float(inp["scale"].min()) and float(inp["scale"].max()) <= 2.0
        want = (torch.baddbmm(t, R, inp["points"].double().transpose(1, 2)).transpose(1, 2)
                - inp["mean"].double()[:, None]) / inp["scale"].double()[:, None, None]
        close(E.tp_reference(inp), want, rtol=1e-9, what="transform_points")
        ev = E.tp_inputs(B, 257, evaluation=True)
        assert float(ev["mean"].abs().max()) == 0 and bool((ev["scale"] == 1).all())


# =====================================================================================================
# branch accounting
# =====================================================================================================
def _source(*path):
    return open(os.path.join(ROOT, *path)).read()


def launcher(text, name):
    """The body of `extern "C" int name(...)` with white space collapsed."""
    start = text.index('extern "C" int %s(' % name)
    end = text.find('\nextern "C"', start + 1)
    return re.sub(r"\s+", " ", text[start:end if end > 0 else len(text)])


def _int(pattern, src):
    found = re.findall(pattern, src)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def launched(src):
    """Kernel names a launcher body can launch: direct launches and the instantiations behind its two macros."""
    names = set(re.findall(r"hipLaunchKernelGGL\(\(?([A-Za-z0-9_]+(?:<[0-9, ]+>)?)", src))
    names |= {"group_norm_pow2_kernel<%s, %s>" % m for m in re.findall(r"ZS_GN_LAUNCH\((\d+), (true|false)\)", src)}
    names |= {"attention_lds_kernel<%s, %s>" % m for m in re.findall(r"ZS_ATT_LDS\((\d+), (\d+)\)", src)}
    return {n for n in names if not n.endswith(("group_norm_pow2_kernel", "attention_lds_kernel"))}   # the macros' own bodies


class Thresholds(object):
    """Read from csrc/nn_ops.hip and csrc/nn_train_norm.hip; the conditions around them are required verbatim, so a
    launcher that changes shape fails here instead of being restated wrongly."""

    def __init__(self):
        ops, train = _source("zeroshape_amd", "csrc", "nn_ops.hip"), _source("zeroshape_amd", "csrc", "nn_train_norm.hip")
        self.src = {n: launcher(ops, n) for n in ("zs_layer_norm", "zs_group_norm_nhwc", "zs_group_norm_nhwc_ws",
                                                  "zs_max_pool_nhwc", "zs_upsample2x_nhwc", "zs_attention_split", "zs_attention")}
        self.src["zs_upsample2x_bwd_nhwc"] = launcher(train, "zs_upsample2x_bwd_nhwc")

        def need(name, snippet):
            assert snippet in self.src[name], "%s no longer reads: %s" % (name, snippet)
        # GroupNorm
        self.gn_block = _int(r"#define ZS_GN_BLOCK (\d+)", ops)
        assert "constexpr int GN_BLOCK = ZS_GN_BLOCK;" in ops
        self.gn_cache_bytes = _int(r"constexpr int GN_CACHE_BYTES = (\d+) \* 1024;", ops) * 1024
        need("zs_group_norm_nhwc", "const int cg = C / groups;")
        need("zs_group_norm_nhwc", "const bool pow2 = (cg & (cg - 1)) == 0 && (long long)HW * cg < (1LL << 30);")
        need("zs_group_norm_nhwc", "if (!pow2 || gn_generic) {")
        need("zs_group_norm_nhwc", "const int vec = cg >= 4 ? 4 : cg;")
        need("zs_group_norm_nhwc", "const size_t bytes = (size_t)HW * cg * sizeof(float);")
        need("zs_group_norm_nhwc", "const bool cache = bytes <= (size_t)GN_CACHE_BYTES;")
        need("zs_group_norm_nhwc", "dim3(batch * groups), dim3(GN_BLOCK)")
        need("zs_group_norm_nhwc_ws", "if (workspace && !no_two &&")
        self.gn_two_launch_bytes = _int(r"sizeof\(float\) >= \(\(size_t\)(\d+) << 20\)", self.src["zs_group_norm_nhwc_ws"]) << 20
        assert "if x.numel() * 4 >= (%d << 20):" % (self.gn_two_launch_bytes >> 20) in _source("zeroshape_amd", "nn", "ops.py")
        # LayerNorm
        need("zs_layer_norm", "const dim3 grid((rows + 3) / 4);")
        self.ln_bounds = [(int(b), int(nv)) for b, nv in re.findall(
            r"if \(\(C & 3\) == 0 && C <= (\d+)\) hipLaunchKernelGGL\(layer_norm_reg_kernel<(\d+)>", self.src["zs_layer_norm"])]
        need("zs_layer_norm", "else hipLaunchKernelGGL(layer_norm_kernel,")
        # max pool, x2 bilinear
        need("zs_max_pool_nhwc", "const size_t quads = (size_t)batch * Hout * Wout * (C / 4);")
        need("zs_max_pool_nhwc", "if ((C & 3) == 0 && quads < (1u << 31)) {")
        need("zs_upsample2x_nhwc", "if ((C & 3) == 0 && 2 * Hin <= 65535 && batch <= 65535 && (long long)2 * Win * (C / 4) < (1LL << 30))")
        need("zs_upsample2x_bwd_nhwc", "if ((C & 3) == 0 && ((reinterpret_cast<size_t>(dy) | reinterpret_cast<size_t>(dx)) & 15) == 0)")
        # attention
        att = self.src["zs_attention_split"]
        need("zs_attention_split", "const dim3 grid(batch * heads, (L + 31) / 32);")
        self.kw_below = _int(r'atoll\(getenv\("ZS_ATT_KW_BELOW"\)\) : (\d+);', att)
        self.kw_min_l = _int(r"if \(\(long long\)grid\.x \* grid\.y < kw_below && L > (\d+)\) \{", att)
        self.lds_min_pairs = _int(r'atoll\(getenv\("ZS_ATT_LDS_MIN_PAIRS"\)\) : (\d+);', att)
        lo_hi = re.findall(r"if \(!no_lds && \(long long\)batch \* heads >= lds_min_pairs && L > (\d+) && L <= (\d+)\) \{", att)
        assert len(lo_hi) == 1, lo_hi
        self.lds_above, self.lds_up_to = int(lo_hi[0][0]), int(lo_hi[0][1])
        pads = set(re.findall(r"if \(L <= (\d+)\) ZS_ATT_LDS\((\d+), (\d+)\); else ZS_ATT_LDS\((\d+), (\d+)\);", att))
        assert len(pads) == 2 and {p[1] for p in pads} == {"32", "64"}, pads
        for small_l, d0, small, d1, big in pads:
            assert d0 == d1 and small_l == small and int(big) == self.lds_up_to, pads
        self.lds_small = int(next(iter(pads))[0])
        need("zs_attention_split", "if (head_dim == 64) hipLaunchKernelGGL(attention_split_kw_kernel<64>,")
        need("zs_attention_split", "if (head_dim == 64) hipLaunchKernelGGL(attention_split_kernel<64>,")
        need("zs_attention", "if (head_dim == 64) hipLaunchKernelGGL(attention_kernel<64>,")


@pytest.fixture(scope="module")
def T():
    return Thresholds()


# ---- the restatement: (launcher, sizes) -> kernel ----
def layer_norm_kernel(T, rows, C):
    for bound, nv in T.ln_bounds:
        if C % 4 == 0 and C <= bound:
            return "layer_norm_reg_kernel<%d>" % nv
    return "layer_norm_kernel"


def group_norm_kernel(T, B, HW, C, groups):
    assert B * HW * C * 4 < T.gn_two_launch_bytes                   # ops.group_norm passes no workspace: one launch
    cg = C // groups
    if cg & (cg - 1) or HW * cg >= 1 << 30:
        return "group_norm_kernel"
    return "group_norm_pow2_kernel<%d, %s>" % (min(4, cg), "true" if HW * cg * 4 <= T.gn_cache_bytes else "false")


def max_pool_kernel(T, B, Ho, Wo, C):
    return "max_pool_quad_kernel" if C % 4 == 0 and B * Ho * Wo * (C // 4) < 1 << 31 else "max_pool_kernel"


def upsample2x_kernel(T, B, Hin, Win, C):
    vec = C % 4 == 0 and 2 * Hin <= 65535 and B <= 65535 and 2 * Win * (C // 4) < 1 << 30
    return "upsample2x_vec_kernel" if vec else "upsample2x_kernel"


def upsample2x_bwd_kernel(T, B, Hin, Win, C):
    return "upsample2x_bwd_kernel<%d>" % (4 if C % 4 == 0 else 1)   # torch's allocations are 16-byte aligned


def attention_split_kernel(T, B, L, heads, d):
    tiles = (L + 31) // 32
    if B * heads * tiles < T.kw_below and L > T.kw_min_l:
        return "attention_split_kw_kernel<%d>" % d
    if B * heads >= T.lds_min_pairs and T.lds_above < L <= T.lds_up_to:
        return "attention_lds_kernel<%d, %d>" % (d, T.lds_small if L <= T.lds_small else T.lds_up_to)
    return "attention_split_kernel<%d>" % d


def attention_kernel(T, B, L, heads, d):
    return "attention_kernel<%d>" % d


# what the element-count guards leave for sizes no test can hold; the accounting asserts that no case comes near them
UNREACHED = [
    "zs_group_norm_nhwc: group_norm_kernel for a power-of-two width when HW x width >= 2^30",
    "zs_group_norm_nhwc_ws: gn_partial_kernel + gn_apply_kernel from 8 MiB on (tests/test_gpu_nn_layers.py has them)",
    "zs_max_pool_nhwc: max_pool_kernel for C % 4 == 0 when the output holds >= 2^31 quads",
    "zs_upsample2x_nhwc: upsample2x_kernel for C % 4 == 0 when 2 Hin > 65535, batch > 65535 or 2 Win C / 4 >= 2^30",
    "zs_upsample2x_bwd_nhwc: upsample2x_bwd_kernel<1> for C % 4 == 0 on a gradient that is not 16-byte aligned",
    "zs_attention, zs_attention_split: the refusal of L > 32 x 65535",
]


def cases_by_kernel(T):
    """launcher -> {kernel: [case, ...]} over every case of the GPU module."""
    hit = collections.defaultdict(lambda: collections.defaultdict(list))
    for C in E.LN_C:
        for rows in E.LN_ROWS:
            hit["zs_layer_norm"][layer_norm_kernel(T, rows, C)].append((rows, C))
    for rows, C in E.LN_ILL_CASES:
        hit["zs_layer_norm"][layer_norm_kernel(T, rows, C)].append((rows, C, "ill"))
    for cfg in E.GN_CASES + [E.GN_ILL_CASE]:
        B, H, W, C, groups = cfg[:5]
        hit["zs_group_norm_nhwc"][group_norm_kernel(T, B, H * W, C, groups)].append(cfg)
    for C in E.POOL_C:
        for H, W in E.POOL_MAPS:
            for k, stride, padding in E.POOL_WINDOWS:
                Ho, Wo = E.pool_out_size(H, k, stride, padding), E.pool_out_size(W, k, stride, padding)
                if min(Ho, Wo) >= 1:
                    hit["zs_max_pool_nhwc"][max_pool_kernel(T, 2, Ho, Wo, C)].append((C, H, W, k, stride, padding))
    for C in E.UP_C:
        for H, W in E.UP_MAPS:
            hit["zs_upsample2x_nhwc"][upsample2x_kernel(T, 2, H, W, C)].append((H, W, C))
            hit["zs_upsample2x_bwd_nhwc"][upsample2x_bwd_kernel(T, 2, H, W, C)].append((H, W, C))
    for c in E.ATT_CASES + [E.ATT_BIG_CASE]:
        hit["zs_attention_split"][attention_split_kernel(T, *c)].append(c)
        hit["zs_attention"][attention_kernel(T, *c)].append(c)
    return hit


def test_every_reachable_kernel_has_a_case(T):
    """Accounting from the code, not an observation of what ran: the launcher conditions are restated above in Python, with
    the thresholds read from the source text (GN_CACHE_BYTES, ZS_GN_BLOCK, the 256 / 512 / 1024 LayerNorm bounds, the
    512-tile and 128-pair attention gates), and every case of the GPU module is mapped through them.  Every kernel a
    launcher names must come out at least once.  The branches behind the 2^30 / 2^31 element-count guards are out of reach
    at test sizes; UNREACHED lists them.  (The process-wide switches ZS_GN_GENERIC, ZS_ATT_NO_LDS, ZS_ATT_KW_BELOW,
    ZS_ATT_LDS_MIN_PAIRS are taken as unset.)"""
    hit = cases_by_kernel(T)
    assert sorted(hit) == sorted(T.src.keys() - {"zs_group_norm_nhwc_ws"})
    for name in sorted(hit):
        reachable = launched(T.src[name])
        for kernel in sorted(reachable):
            print("%s -> %s: %d cases, e.g. %s" % (name, kernel, len(hit[name][kernel]), hit[name][kernel][:1]))
        assert set(hit[name]) <= reachable, (name, sorted(set(hit[name]) - reachable))      # the restatement names real kernels
        assert not reachable - set(hit[name]), "%s: no case reaches %s" % (name, sorted(reachable - set(hit[name])))
    assert launched(T.src["zs_group_norm_nhwc_ws"]) == {"gn_partial_kernel", "gn_apply_kernel"}     # out of scope here
    for line in UNREACHED:
        print("unreached: " + line)
    assert T.ln_bounds == [(256, 1), (512, 2), (1024, 4)] and all(b == 256 * nv for b, nv in T.ln_bounds)
    assert (T.kw_below, T.lds_min_pairs) == (512, 128)
    assert T.gn_cache_bytes == 112 * 1024 and T.gn_block == 512


def test_cases_sit_on_both_sides_of_every_threshold(T):
    # LayerNorm: the last C of every register kernel and the first of the next; C % 4 != 0 below the first bound
    for bound, nv in T.ln_bounds:
        assert bound in E.LN_C and bound + 4 in E.LN_C, bound
    assert any(C % 4 and C < T.ln_bounds[0][0] for C in E.LN_C) and any(C % 4 and C > T.ln_bounds[0][0] for C in E.LN_C)
    assert {1, 3, 4, 5} <= set(E.LN_ROWS)                           # around the four rows of a workgroup
    # GroupNorm: per vector width one slice above GN_CACHE_BYTES whose next smaller square map is below it, and is a case too
    sides = collections.defaultdict(set)
    for B, H, W, C, groups, relu, res in E.GN_CASES:
        cg = C // groups
        if cg & (cg - 1):
            assert H * W * cg % T.gn_block                          # the generic kernel's last sweep is ragged
            continue
        cached = H * W * cg * 4 <= T.gn_cache_bytes
        sides[(cg, cached)].add((H, W))
        assert B * H * W * C * 4 < T.gn_two_launch_bytes
        assert H * W * cg // min(4, cg) > T.gn_block and H * W * cg // min(4, cg) % T.gn_block      # several sweeps, the last ragged
    for cg in (1, 2, 4, 16):
        (above,), (below,) = sides[(cg, False)], sides[(cg, True)]
        assert above[0] == above[1] and below == (above[0] - 1, above[1] - 1), (cg, above, below)
    assert E.GN_ILL_CASE[:5] in [c[:5] for c in E.GN_CASES] and group_norm_kernel(T, *_gn_sizes(E.GN_ILL_CASE)).endswith("false>")
    assert {c[5:] for c in E.GN_CASES} == {(True, False), (False, True), (True, True), (False, False)}
    # attention: both sides of the staged kernel's L range and of its two paddings at >= 128 pairs; a single tile, one key
    # short of it and one beyond it below 128 pairs
    many = {c[1] for c in E.ATT_CASES if c[0] * c[2] >= T.lds_min_pairs and c[3] == 32}
    assert {T.lds_above, T.lds_above + 1, T.lds_small, T.lds_small + 1, T.lds_up_to, T.lds_up_to + 1} <= many
    assert min(c[0] * c[2] for c in E.ATT_CASES if c[0] * c[2] >= T.lds_min_pairs) == T.lds_min_pairs
    for d in (32, 64):
        assert {1, 31, 32, 33, 64} <= {c[1] for c in E.ATT_CASES if c[0] * c[2] < T.lds_min_pairs and c[3] == d}
    assert E.ATT_BIG_CASE[1] == T.lds_up_to + 1
    # pooling, global mean, x2 bilinear, transform_points: the sets the kernels' tiles call for
    assert {1, 3, 5, 6, 64} == set(E.POOL_C) and {1, 63, 64, 65, 100, 130} == set(E.MEAN_C)
    assert {1, 2, 3, 5, 49} == {h * w for h, w in E.MEAN_MAPS}
    assert {(1, 1), (2, 2), (2, 7), (3, 2), (5, 1)} == set(E.UP_MAPS) and {1, 3, 4, 8} == set(E.UP_C)
    assert {1, 255, 256, 257, 1000} == set(E.TP_N) and {1, 3} == set(E.TP_B)


def _gn_sizes(cfg):
    B, H, W, C, groups = cfg[:5]
    return B, H * W, C, groups
