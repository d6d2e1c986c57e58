"""Block 0's point-side q/k/v as a rank-4 table (zeroshape_amd/program.py: block0_window; csrc/sdf_decoder_split.hip:
BLOCK 0 TABLE, which the compact block-0 stream is built from) - the parts that need no GPU.

  * the identity: the table, evaluated in fp32 with five fmas per value, gives LN1 + qkv Linear of point_proj(xyz);
  * the weight stream's schedule when every block runs its q/k/v GEMMs (block 1 always, block 0 as the fallback): a
    wave-by-wave model of the staging (per-wave source pointer, the pos-7 step staging chunk n + 2) consumes the program's
    K-blocks in order."""
import numpy as np
import pytest

from zeroshape_amd import program as P

F = np.float32


def _points():
    rs = np.random.RandomState(11)
    corners = np.array([[x, y, z] for x in (-1.5, 1.5) for y in (-1.5, 1.5) for z in (-1.5, 1.5)], np.float32)
    special = np.concatenate([np.zeros((1, 3), np.float32), corners, np.array([[1e-4, 0, 0]], np.float32)])
    return np.concatenate([special, rs.uniform(-1.5, 1.5, size=(3000, 3)).astype(np.float32)])


def _kernel_qkv(window, sd, pts):
    """q/k/v rows [n, 768] (attn.qkv.weight row order) from the window, in the split kernel's fp32: point_proj op for op
    (xyz_affine), ln_stats op for op, then five fmas per value - the fp32 evaluation of rstd (T p~) + c.  float64 products
    of float32 operands rounded to float32 ARE the fused multiply-adds for these magnitudes (the 24 x 24-bit product is
    exact in 53 bits; the one rounding of the sum to float32 after an exact-product double add differs from fmaf only by
    double rounding, far below the tolerance)."""
    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    Wp = sd["point_proj.proj.weight"].astype(F)
    bp = sd["point_proj.proj.bias"].astype(F)
    x, y, z = (pts[:, i:i + 1].astype(F) for i in range(3))
    ones = np.ones_like(x)
    pf = fma(ones * Wp[None, :, 2], z, fma(ones * Wp[None, :, 1], y, fma(ones * Wp[None, :, 0], x, ones * bp[None, :])))
    mean = (pf.sum(1, dtype=F) * F(1.0 / 256.0)).astype(F)
    d = (pf - mean[:, None]).astype(F)
    var = (d * d).sum(1, dtype=F)
    rstd = (F(1.0) / np.sqrt(var * F(1.0 / 256.0) + F(1e-6), dtype=F)).astype(F)[:, None]
    xr, yr, zr = (x * rstd).astype(F), (y * rstd).astype(F), (z * rstd).astype(F)
    c = window[P.B0_C:P.B0_T].reshape(24, 2, 16)                      # [tile][hi][r]
    T = window[P.B0_T:].reshape(24, 2, 16, 4)
    out = np.zeros((pts.shape[0], 3 * P.C), F)
    for h in range(P.HEADS):
        for part in range(3):
            for hi in range(2):
                for r in range(16):
                    w = T[3 * h + part, hi, r]
                    n = np.ones_like(x)
                    v = fma(n * w[2], zr, fma(n * w[1], yr, fma(n * w[0], xr, fma(n * w[3], rstd, n * c[3 * h + part, hi, r]))))
                    out[:, part * P.C + h * P.HD + P.row(r, hi)] = v[:, 0]
    return out, pf


def _direct_qkv(sd, pts):
    """fp64 LayerNorm + Linear of the fp32 point rows."""
    g = lambda k: np.asarray(sd[k], np.float64)
    pf = pts.astype(np.float64) @ g("point_proj.proj.weight").T + g("point_proj.proj.bias")
    mu = pf.mean(1, keepdims=True)
    var = ((pf - mu) ** 2).mean(1, keepdims=True)
    ln = (pf - mu) / np.sqrt(var + 1e-6) * g("blocks_attn.0.norm1.weight") + g("blocks_attn.0.norm1.bias")
    return ln @ g("blocks_attn.0.attn.qkv.weight").T + g("blocks_attn.0.attn.qkv.bias")


def _gemm_qkv(sd, pf):
    """The same rows from the arithmetic the table replaces (the split kernel's LN1 + three GEMMs per head), restated: fp32
    LayerNorm with the kernel's fp32 mean / rstd, activations and weights split into fp16 hi + lo (round to nearest even),
    and per K-block of 16 features the three MFMAs A_lo B_hi, A_hi B_lo, A_hi B_hi accumulated in fp32 on the bias (each
    MFMA's 16 products summed exactly, then one fp32 rounding)."""
    def split(x):
        hi = P.f16_round(x)[1]
        lo = P.f16_round((x - hi).astype(F))[1]
        return hi.astype(np.float64), lo.astype(np.float64)
    mean = (pf.sum(1, dtype=F) * F(1.0 / 256.0)).astype(F)
    d = (pf - mean[:, None]).astype(F)
    var = (d * d).sum(1, dtype=F)
    rstd = (F(1.0) / np.sqrt(var * F(1.0 / 256.0) + F(1e-6), dtype=F)).astype(F)[:, None]
    g, b = sd["blocks_attn.0.norm1.weight"].astype(F), sd["blocks_attn.0.norm1.bias"].astype(F)
    t = ((d * rstd).astype(F).astype(np.float64) * g + b).astype(F)
    bh, bl = split(t)
    ah, al = split(sd["blocks_attn.0.attn.qkv.weight"].astype(F))
    acc = np.broadcast_to(sd["blocks_attn.0.attn.qkv.bias"].astype(F), (pf.shape[0], 3 * P.C)).copy()
    for kb in range(2 * P.NT):                        # a K-block holds 16 consecutive features
        k = slice(16 * kb, 16 * kb + 16)
        for a_, b_ in ((al, bh), (ah, bl), (ah, bh)):
            acc = (acc.astype(np.float64) + b_[:, k] @ a_[:, k].T).astype(F)
    return acc


@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_table_reproduces_ln1_and_qkv(seeded_sd, gain):
    """Bound: 2e-6 absolute at the seeded weights' scale (max |q, k, v| = 2.85), i.e. 2e-6 * max(1, max |q, k, v| / 2.85): every
    error term of an fp32 evaluation (the rounding of rstd, of the table and of the five fmas) is relative to the values, and
    with the attention weights x4 one fp32 ulp at |v| = 11.6 is already 9.5e-7.  The relative form is justified here, not
    assumed: the arithmetic the table replaces (_gemm_qkv) is evaluated on the same points and the table must be no worse than
    it, in the maximum and in the mean.  Measured by this test against the direct fp64 LN1 + Linear (3,010 points):
        gain 1: table max 1.34e-6 (mean 2.2e-7), GEMMs max 1.55e-6 (mean 2.4e-7), max |q, k, v| 2.85, bound 2e-6
        gain 4: table max 2.45e-6 (mean 2.8e-7), GEMMs max 5.23e-6 (mean 4.2e-7), max |q, k, v| 11.6, bound 8.1e-6
    (both share the kernel's fp32 rstd, whose rounding alone is ~1e-7 of the value)."""
    sd = {k: np.asarray(v, np.float32).copy() for k, v in seeded_sd.items()}
    sd["blocks_attn.0.attn.qkv.weight"] *= F(gain)
    pts = _points()
    window = P.block0_window(P.split_program(P.pack_program(sd)))
    assert window.dtype == np.float32 and window.shape == (P.B0_WINDOW_FLOATS,) == (4096,)
    np.testing.assert_array_equal(window[:P.C], P.rowparam(sd["blocks_attn.0.attn.proj.bias"]))
    got, pf = _kernel_qkv(window, sd, pts)
    want = _direct_qkv(sd, pts)
    e_tab, e_gemm = np.abs(got - want), np.abs(_gemm_qkv(sd, pf) - want)
    vmax = float(np.abs(want).max())
    bound = 2e-6 * max(1.0, vmax / 2.85)
    print("gain %g: table max %.3g mean %.3g | GEMMs max %.3g mean %.3g | max |q, k, v| = %.3g, bound %.3g" %
          (gain, e_tab.max(), e_tab.mean(), e_gemm.max(), e_gemm.mean(), vmax, bound))
    assert float(e_tab.max()) < bound
    assert float(e_tab.max()) <= float(e_gemm.max()) and float(e_tab.mean()) <= float(e_gemm.mean())


def _stream_model():
    """The K-blocks the four waves multiply, in order, from a model of AStream: two buffers of one chunk (8 K-blocks), wave w
    stages K-blocks 2 w, 2 w + 1 of a chunk from ITS pointer gsrc[w]; init stages two chunks; the step at chunk position 7
    stages the chunk after next into the buffer just consumed.  All sizes in K-blocks."""
    CK = 8
    gsrc = [2 * w for w in range(4)]
    bufs = [[None] * CK, [None] * CK]

    def stage(buf):
        for w in range(4):
            buf[2 * w], buf[2 * w + 1] = gsrc[w], gsrc[w] + 1
            gsrc[w] += CK
    stage(bufs[0])
    stage(bufs[1])
    consumed, pos = [], [0]

    def step(expect_pos):
        assert pos[0] == expect_pos                       # the kernel's positions are compile-time constants
        consumed.append(bufs[0][pos[0]])
        if pos[0] == CK - 1:
            stage(bufs[0])
            bufs[0], bufs[1] = bufs[1], bufs[0]
        pos[0] = (pos[0] + 1) % CK

    for blk in range(P.BLOCKS):
        for hd in range(P.HEADS):
            Ppos = 0 if hd % 2 == 0 else 4
            for _ in range(3):
                for kb in range(16):
                    step((Ppos + kb) % CK)
            for lt in range(P.LT):                        # attn_tile: S at pos0, o at pos0 + 2; tiles alternate P, P + 4
                p0 = Ppos if lt % 2 == 0 else (Ppos + 4) % CK
                for j in range(4):
                    step((p0 + j) % CK)
            for nt in range(P.NT):
                for j in range(2):
                    step((Ppos + 4 + 2 * nt + j) % CK)
        for _ in range(P.HT * 32):                        # the MLP section: chunk-aligned, sequential
            step(pos[0])
    n_impl = P.G_IMPL // 2
    for _ in range(n_impl):
        step(pos[0])
    assert pos[0] == 0
    return consumed


def test_schedule_model_consumes_the_list():
    assert _stream_model() == list(range(P.KB_TOTAL))

