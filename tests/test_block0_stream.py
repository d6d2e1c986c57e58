"""Block 0 from its compact stream (zeroshape_amd/program.py: block0_stream and friends; csrc/sdf_decoder_split.hip:
BLOCK 0 STREAM) - the parts that need no GPU.

  * the identity and its accuracy: the packed rank-5 operands, multiplied as ONE fp16 MFMA each (tests/mfma_emulator.py),
    give block 0's q, k, v and its point-to-latent logits; against a direct fp64 LN1 -> Linear -> K q they are no worse
    than the GEMM arithmetic they replace, in the maximum and in the mean;
  * the weight stream's schedule: a wave-by-wave model of the staging delivers the compact stream's 272 slots, then the
    program's K-blocks from 736 on, once each and in order, with every chunk position the compile-time constant the kernel
    uses;
  * the fit predicate at its boundary."""
import numpy as np
import pytest

from zeroshape_amd import program as P
from tests import mfma_emulator as E
from tests.test_block0_tables import _direct_qkv, _gemm_qkv, _points

F = np.float32
C_LOG = P.HD ** -0.5 * P.LOG2E


def _kernel_u(sd, pts):
    """u = (rstd x, rstd y, rstd z, rstd, 1) [n, 5] fp32 and the fp32 point rows, op for op as the split kernel forms them
    (xyz_affine, ln_stats; see tests/test_block0_tables.py: _kernel_qkv)."""
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
    u = np.concatenate([(x * rstd).astype(F), (y * rstd).astype(F), (z * rstd).astype(F), rstd, np.ones_like(rstd)], axis=1)
    return u, pf


def _as_f64(bits16):
    return np.ascontiguousarray(bits16).view(np.float16).astype(np.float64)


def _rank5_mfma(a_rows, u):
    """[n points][32 rows] fp32: ONE emulated v_mfma_f32_32x32x16_f16 per wave tile of 32 points on the packed operands (the
    16 products summed exactly, one rounding to fp32: the accumulator starts at zero)."""
    n = u.shape[0]
    A = _as_f64(P.pack_rank5_a(a_rows))
    out = np.zeros((n, 32), F)
    inv = np.empty(32, np.int64)
    inv[P.ROW_TABLE.reshape(-1)] = np.arange(32)             # row t of the tile sits in (hi, r) = divmod(inv[t], 16)
    for w in range(0, n, 32):
        B = _as_f64(P.pack_rank5_b(u[w:w + 32]))
        acc = E.mfma16(A, B, np.zeros((16, 64))).astype(F)  # [r][lane]
        both = np.concatenate([acc[:, :32], acc[:, 32:]], axis=0)   # [hi * 16 + r][point]
        out[w:w + 32] = both[inv].T
    return out


def _kv(seed):
    rs = np.random.RandomState(seed)
    return {(blk, h): (rs.standard_normal((P.L, P.HD)).astype(F), rs.standard_normal((P.L, P.HD)).astype(F))
            for blk in range(P.BLOCKS) for h in range(P.HEADS)}


def _k_halves(words, h):
    """K rows of block 0, head h as the split program holds them: (hi, lo) float64 [224, 32]."""
    hi, lo = np.zeros((P.LT * 32, P.HD)), np.zeros((P.LT * 32, P.HD))
    for lt in range(P.LT):
        for j in range(2):
            kb = h * P.KB_HEAD + P.KB_QKV_HEAD + 4 * lt + j
            v = np.ascontiguousarray(words[kb * P.KB_WORDS:(kb + 1) * P.KB_WORDS]).view(np.float16).reshape(2, 64, 8)
            rows, cols = 32 * lt + P.LANE_I[:, None], P.ROW_TABLE[P.LANE_HI][:, 8 * j:8 * j + 8]
            hi[rows, cols], lo[rows, cols] = v[0], v[1]
    return hi, lo


def _gemm_logits(q, kh, kl):
    """The logits the way the program arm forms them: S = K q on split operands, two K-blocks of three MFMAs, fp32
    accumulation from zero, then the fp32 factor c (attn_tile)."""
    qh, ql = E._split_f16(q)
    acc = np.zeros((q.shape[0], kh.shape[0]), F)
    for j in range(2):
        f = np.concatenate([P.ROW_TABLE[0][8 * j:8 * j + 8], P.ROW_TABLE[1][8 * j:8 * j + 8]])
        for a_, b_ in ((kl, qh), (kh, ql), (kh, qh)):
            acc = (acc.astype(np.float64) + b_[:, f] @ a_[:, f].T).astype(F)
    return (acc.astype(np.float64) * np.float64(F(P.HD ** -0.5) * F(P.LOG2E))).astype(F)


@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_packed_operands_reproduce_qkv_and_logits(seeded_sd, gain):
    """Against the direct fp64 LN1 -> Linear -> c K q on the inputs of test_table_reproduces_ln1_and_qkv (3,010 points with the
    origin, the corners and a point 1e-4 from the origin; K rows: seeded standard normal, taken as the split program holds
    them), the packed arithmetic must be no worse than the GEMM arithmetic it replaces - q/k/v: LN1 + three split GEMMs;
    logits: those q through the split K q GEMM - in the maximum and in the mean.  The figures are printed before the
    assertions.  Measured by this test (max / mean):
        gain 1: q/k/v packed 1.37e-6 / 2.26e-7, GEMMs 1.55e-6 / 2.37e-7; logits packed 2.44e-6 / 3.24e-7, GEMMs 2.50e-6 / 3.46e-7
        gain 4: logits packed 5.29e-6 / 4.61e-7, GEMMs 6.21e-6 / 6.65e-7 (max |S| 18.5)
    (with the remainders unscaled, program.B0S_LO_SCALE = 1, the q/k/v mean is 2.73e-7 and the test fails: fp16 subnormals)."""
    sd = {k: np.asarray(v, np.float32).copy() for k, v in seeded_sd.items()}
    sd["blocks_attn.0.attn.qkv.weight"] *= F(gain)
    pts = _points()
    pad = (-pts.shape[0]) % 32
    pts = np.concatenate([pts, pts[:pad]])
    words = P.split_program(P.pack_program(sd, kv=_kv(5)))
    rows = P.block0_rank5_rows(words)
    u, pf = _kernel_u(sd, pts)
    want = _direct_qkv(sd, pts)
    gemm = _gemm_qkv(sd, pf)
    got = np.zeros_like(gemm)
    e_s_pack, e_s_gemm, smax = [], [], 0.0
    for h in range(P.HEADS):
        for part in range(3):
            got[:, part * P.C + h * P.HD:part * P.C + (h + 1) * P.HD] = _rank5_mfma(rows[h, part], u)
        kh, kl = _k_halves(words, h)
        s_want = C_LOG * want[:, h * P.HD:(h + 1) * P.HD] @ (kh + kl).T                       # [n, 224], float64
        s_pack = np.concatenate([_rank5_mfma(rows[h, 3 + lt], u) for lt in range(P.LT)], axis=1)
        s_gemm = _gemm_logits(gemm[:, h * P.HD:(h + 1) * P.HD], kh, kl)
        e_s_pack.append(np.abs(s_pack - s_want)[:, :P.L])
        e_s_gemm.append(np.abs(s_gemm - s_want)[:, :P.L])
        smax = max(smax, float(np.abs(s_want).max()))
        assert not s_pack[:, P.L:].any()                                                    # padding rows: U = 0
    e_pack, e_gemm = np.abs(got - want), np.abs(gemm - want)
    e_s_pack, e_s_gemm = np.stack(e_s_pack), np.stack(e_s_gemm)
    print("gain %g q/k/v: packed max %.3g mean %.3g | GEMMs max %.3g mean %.3g | max |q, k, v| = %.3g" %
          (gain, e_pack.max(), e_pack.mean(), e_gemm.max(), e_gemm.mean(), float(np.abs(want).max())))
    print("gain %g logits (log2 domain): packed max %.3g mean %.3g | GEMMs max %.3g mean %.3g | max |S| = %.3g" %
          (gain, e_s_pack.max(), e_s_pack.mean(), e_s_gemm.max(), e_s_gemm.mean(), smax))
    assert float(e_pack.max()) <= float(e_gemm.max()) and float(e_pack.mean()) <= float(e_gemm.mean())
    assert float(e_s_pack.max()) <= float(e_s_gemm.max()) and float(e_s_pack.mean()) <= float(e_s_gemm.mean())


def test_stream_mirror_layout(seeded_sd):
    """Copies are the program's K-blocks word for word; a packed slot holds its two operands; the slot list is the
    documented order."""
    sd = {k: np.asarray(v, np.float32) for k, v in seeded_sd.items()}
    words = P.split_program(P.pack_program(sd, kv=_kv(6)))
    stream = P.block0_stream(words).reshape(P.B0S_KB, P.KB_WORDS)
    rows = P.block0_rank5_rows(words)
    slots = P.block0_stream_slots()
    assert [s[0] for s in slots].count("pack") == 5 and len(slots) == 34 and P.B0S_WORDS * 4 == 544 * 1024
    assert sorted(op for s in slots if s[0] == "pack" for op in s[1:]) == list(range(10))
    copies = [s[1] for s in slots if s[0] == "copy"]
    assert copies == [48 + 4 * lt + 2 + j for lt in range(7) for j in range(2)][:13] + list(range(76, 92))
    for h in (0, 7):
        for i, s in enumerate(slots):
            got = stream[h * 34 + i]
            if s[0] == "copy":
                kb = h * P.KB_HEAD + s[1]
                assert np.array_equal(got, words[kb * P.KB_WORDS:(kb + 1) * P.KB_WORDS])
            else:
                for half, op in enumerate(s[1:]):
                    assert np.array_equal(got[half * 256:(half + 1) * 256].view(np.uint16).reshape(64, 8),
                                          P.pack_rank5_a(rows[h, op]))
    # every operand's S tile comes before the V K-blocks that consume its probabilities
    for lt in range(P.LT):
        first_v = min(i for i, s in enumerate(slots) if s == ("copy", 48 + 4 * lt + 2))
        assert any(s[0] == "pack" and 3 + lt in s[1:] for s in slots[:first_v])


def _stream_model():
    """The slots the four waves multiply, in order, from a model of AStream on the compact-stream arm: two buffers of one chunk
    (8 slots), wave w stages slots 2 w, 2 w + 1 of a chunk from ITS pointer; init stages two chunks of the compact stream; the
    step at chunk position 7 stages the chunk after next into the buffer just consumed; in front of head 7's proj loop every
    wave's pointer moves to the program's K-block 736 (AStream::seek).  step(expect) asserts the position the kernel passes as
    a compile-time constant."""
    CK = 8
    gsrc = [("b0", 2 * w) for w in range(4)]
    bufs = [[None] * CK, [None] * CK]

    def stage(buf):
        for w in range(4):
            space, i = gsrc[w]
            buf[2 * w], buf[2 * w + 1] = (space, i), (space, i + 1)
            gsrc[w] = (space, i + CK)
    stage(bufs[0])
    stage(bufs[1])
    consumed, pos = [], [0]

    def step(expect_pos):
        assert pos[0] == expect_pos
        consumed.append(bufs[0][pos[0]])
        if pos[0] == CK - 1:
            stage(bufs[0])
            bufs[0], bufs[1] = bufs[1], bufs[0]
        pos[0] = (pos[0] + 1) % CK
    for blk in range(P.BLOCKS):
        for hd in range(P.HEADS):
            if blk == 0:
                Ppos = (2 * hd) % CK                          # the kernel instantiates head bodies for P = 0, 2, 4, 6
                step(Ppos)                                    # [q | k]
                step((Ppos + 1) % CK)                         # [v | U0]
                for j in range(2):
                    step((Ppos + 2 + j) % CK)                 # PV 0
                for i in range(3):
                    step((Ppos + 4 + 5 * i) % CK)             # [U(2i+1) | U(2i+2)]
                    for j in range(2):
                        step((Ppos + 5 + 5 * i + j) % CK)
                    for j in range(2 if i < 2 else 1):        # latent tile 6: one K-block
                        step((Ppos + 7 + 5 * i + j) % CK)
                if hd == P.HEADS - 1:
                    assert Ppos == 6 and pos[0] == 0          # proj of head 7 = the compact stream's last two chunks
                    for w in range(4):
                        assert gsrc[w] == ("b0", P.B0S_KB + 2 * w)
                        gsrc[w] = ("prog", P.HEADS * P.KB_HEAD + 2 * w)
                for nt in range(P.NT):
                    for j in range(2):
                        step((Ppos + 18 + 2 * nt + j) % CK)
            else:
                Ppos = 0 if hd % 2 == 0 else 4
                for _ in range(3):
                    for kb in range(16):
                        step((Ppos + kb) % CK)
                for lt in range(P.LT):
                    p0 = Ppos if lt % 2 == 0 else (Ppos + 4) % CK
                    for j in range(4):
                        step((p0 + j) % CK)
                for nt in range(P.NT):
                    for j in range(2):
                        step((Ppos + 4 + 2 * nt + j) % CK)
        assert pos[0] == 0
        for _ in range(P.HT * 32):
            step(pos[0])
    for _ in range(P.G_IMPL // 2):
        step(pos[0])
    assert pos[0] == 0
    return consumed


def test_schedule_model_consumes_compact_stream_then_program():
    got = _stream_model()
    want = P.split_consumed_slots_b0_stream()
    assert len(want) == 4464 and want[:272] == [("b0", i) for i in range(272)]
    assert want[272:] == [("prog", kb) for kb in range(736, 4928)]
    assert got == want
    assert [kb for _, kb in want[272:]] == list(range(736, P.KB_TOTAL))
    assert P.SPLIT_MFMAS_B0_STREAM == 13352 == 8 * 97 + 3 * (4928 - 736)


def test_fit_predicate_boundary():
    per_image = 16 * 1024 + 544 * 1024
    n = P.SLAB_REGION_BYTES // per_image
    assert P.SLAB_REGION_BYTES == 96 * 1024 * 1024 and n == 175
    assert P.block0_stream_fit(0) and P.block0_stream_fit(1) and P.block0_stream_fit(n) and not P.block0_stream_fit(n + 1)
    assert n * per_image <= P.SLAB_REGION_BYTES < (n + 1) * per_image
