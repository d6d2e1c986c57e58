"""Host-side packer: reference ``impl_network`` state_dict -> "decoder program".

The fused decoder kernel (csrc/sdf_decoder.hip) keeps every activation of a
32-point tile in registers in the accumulator layout of
``v_mfma_f32_32x32x2_f32`` and computes each layer TRANSPOSED,

    Y^T[n, t] = sum_k W[n, k] * X^T[k, t]        (n = feature, t = point)

so that the output registers of one layer are, unchanged, the B operands of the
next (no LDS round trip, no transposes).  What remains to be fed is the A operand
(weights): one fp32 per lane per MFMA.  This module lays every weight of the model
out as the exact sequence of A operands the kernel consumes, so the kernel's
weight access is ONE linear stream of coalesced 16-byte loads.

Layout facts (cdna_hip_programming.md section 3):
  lane l of a wave supplies  A[i = l & 31][k = l >> 5]  and  B[k = l >> 5][j = l & 31];
  accumulator register r of lane l holds  D[row(r, l >> 5)][l & 31],
  row(r, hi) = (r & 3) + 8 * (r >> 2) + 4 * hi.
Hence an activation tile (32 features x 32 points) lives in 16 registers; register r
holds feature row(r, 0) in lanes 0-31 and row(r, 1) = row(r, 0) + 4 in lanes 32-63,
and using register r as the B operand contracts over exactly those two features.
The matching A "record" (64 floats) for output tile nt, input tile kt, register r is
    rec[l] = W[32 * nt + (l & 31)][32 * kt + row(r, l >> 5)].
Four consecutive records are interleaved per lane into one "group" (1 KiB):
    group[l][j] = rec_{4g + j}[l]         -> one global_load_dwordx4 per lane per 4 MFMAs.

Two buffers are produced:
  * ``recs``   - the record stream (per image; the attention K/V records in it are
                 written per image by the prologue kernel, csrc/sdf_prologue.hip);
  * ``params`` - small per-feature vectors (biases, LayerNorm affine, the 3-wide
                 xyz columns) in "row-param" order [tile][hi][r], staged in LDS.
and, for the prologue, ``lat_params`` (latent-path weights, transposed [K][N]).

Reference semantics: model/shape/implicit.py:251-288 (see oracle/decoder_ref.py).
"""
import numpy as np

# architecture constants of options/shape.yaml:19-44 (the kernel is specialised for them)
C = 256          # channels
NT = C // 32     # 8 feature tiles
HEADS = 8
HD = 32          # head dim == one feature tile
L = 197          # latent tokens
LT = 7           # latent tiles of 32 (224 >= 197; rows >= 197 are zero / masked)
HID = 1024
HT = HID // 32   # 32 hidden tiles
BLOCKS = 2
MLP_LAYERS = 9   # impl_mlp.layers.0..8
SKIP_IN = (2, 4, 6)
GROUP_FLOATS = 256          # 4 records x 64 lanes
RING = 8                    # groups the kernel prefetches ahead (tail padding)

LANE = np.arange(64)
LANE_I = LANE & 31
LANE_HI = LANE >> 5


def row(r, hi):
    return (r & 3) + 8 * (r >> 2) + 4 * hi


# feature index held by (tile-local) register r in lane-half hi, for r = 0..15
ROW_TABLE = np.array([[row(r, hi) for r in range(16)] for hi in range(2)])  # [hi][r]


# ----------------------------------------------------------------------------- #
# record stream
# ----------------------------------------------------------------------------- #
def _records_linear(W, nt, kt):
    """16 records [16, 64] of W (out x in) for output tile nt / input tile kt."""
    rows = 32 * nt + LANE_I                                   # [64]
    cols = 32 * kt + ROW_TABLE[LANE_HI][:, :].T               # [16, 64]: row(r, hi(l))
    return W[rows[None, :], cols]


def _interleave(recs):
    """[n_rec, 64] -> groups [n_rec / 4, 64, 4] flattened."""
    n = recs.shape[0]
    assert n % 4 == 0
    return recs.reshape(n // 4, 4, 64).transpose(0, 2, 1).reshape(-1)


def records_for_linear(W, n_out_tiles=None, k_tiles=None):
    """Records of a whole linear layer in consumption order: for nt: for kt: for r."""
    W = np.asarray(W, np.float32)
    n_out_tiles = W.shape[0] // 32 if n_out_tiles is None else n_out_tiles
    k_tiles = W.shape[1] // 32 if k_tiles is None else k_tiles
    out = [_records_linear(W, nt, kt) for nt in range(n_out_tiles) for kt in range(k_tiles)]
    return np.concatenate(out, axis=0)


def kv_records(K_h, V_h):
    """Attention records of ONE head: for lt: [16 K records][16 V records].
    K_h, V_h: [197, 32] fp32.
      K record (lt, r): A[i = latent row][k = head dim]  = K[32lt + (l&31)][row(r, l>>5)]
      V record (lt, r): A[i = head dim][k = latent row]  = V[32lt + row(r, l>>5)][l&31]
    rows >= 197 are zero (their logits are masked to -inf in the kernel)."""
    Kp = np.zeros((LT * 32, HD), np.float32)
    Vp = np.zeros((LT * 32, HD), np.float32)
    Kp[:L], Vp[:L] = K_h, V_h
    out = []
    for lt in range(LT):
        krec = Kp[(32 * lt + LANE_I)[None, :], ROW_TABLE[LANE_HI].T]            # [16, 64]
        vrec = Vp[32 * lt + ROW_TABLE[LANE_HI].T, LANE_I[None, :]]              # [16, 64]
        out += [krec, vrec]
    return np.concatenate(out, axis=0)                                           # [224, 64]


# groups per section (1 group = 4 records = 4 MFMAs per wave)
G_QKV_HEAD = 3 * NT * 4          # 96: q, k, v tiles of one head (8 input tiles x 4 groups)
G_KV_HEAD = LT * 8               # 56
G_PROJ_HEAD = NT * 4             # 32
G_HEAD = G_QKV_HEAD + G_KV_HEAD + G_PROJ_HEAD   # 184
G_MLP_TILE = NT * 4 + NT * 4     # 64: fc1 tile (32) + fc2 slice (32)
G_BLOCK = HEADS * G_HEAD + HT * G_MLP_TILE      # 3520
G_IMPL_PLAIN = NT * NT * 4       # 256
G_IMPL_SKIP = 2 * G_IMPL_PLAIN   # 512
G_IMPL = G_IMPL_PLAIN * 5 + G_IMPL_SKIP * 3     # layers 0,1,3,5,7 plain; 2,4,6 skip
G_TOTAL = BLOCKS * G_BLOCK + G_IMPL             # 9856 groups = 39424 MFMAs per 32 points
REC_FLOATS = (G_TOTAL + RING) * GROUP_FLOATS     # record stream incl. prefetch tail padding
PARAM_FLOATS = 13824                             # params section (13584 used), multiple of 256
PROGRAM_FLOATS = REC_FLOATS + PARAM_FLOATS       # one per-image program: [records | params]
PROGRAM_BYTES = PROGRAM_FLOATS * 4


def kv_group_offset(blk, head):
    """First group of the K/V records of (block, head) inside the record stream."""
    return blk * G_BLOCK + head * G_HEAD + G_QKV_HEAD


def pack_records(sd, kv=None):
    """state_dict (numpy fp32) -> record stream [PROGRAM_FLOATS] fp32.
    ``kv``: optional {(blk, head): (K_h [197,32], V_h [197,32])}; zeros when absent
    (the prologue kernel fills them per image on the device)."""
    out = []
    for blk in range(BLOCKS):
        p = "blocks_attn.%d." % blk
        Wqkv = np.asarray(sd[p + "attn.qkv.weight"], np.float32)      # [768, 256]
        Wproj = np.asarray(sd[p + "attn.proj.weight"], np.float32)    # [256, 256]
        W1 = np.asarray(sd[p + "mlp.fc1.weight"], np.float32)         # [1024, 256]
        W2 = np.asarray(sd[p + "mlp.fc2.weight"], np.float32)         # [256, 1024]
        for h in range(HEADS):
            for part in range(3):                                      # q, k, v rows of head h
                Wt = Wqkv[part * C + h * HD: part * C + (h + 1) * HD]  # [32, 256]
                out.append(records_for_linear(Wt))                     # 128 records
            if kv is not None:
                out.append(kv_records(*kv[(blk, h)]))
            else:
                out.append(np.zeros((G_KV_HEAD * 4, 64), np.float32))
            out.append(records_for_linear(Wproj[:, h * HD:(h + 1) * HD]))  # for nt: 16 records
        for ht in range(HT):
            out.append(records_for_linear(W1[ht * 32:(ht + 1) * 32]))      # fc1 tile: 128 records
            out.append(records_for_linear(W2[:, ht * 32:(ht + 1) * 32]))   # fc2 slice: for nt: 16
    # impl_mlp, in the order the kernel runs it: layer 0 (feat columns), then the feat
    # halves of the three skip layers ("Z" partial products, computed while feat is still in
    # registers and parked in the per-wave workspace), then layers 1..7 with only the
    # x columns left in the skip layers.
    Wl = [np.asarray(sd["impl_mlp.layers.%d.weight" % l], np.float32) for l in range(MLP_LAYERS)]
    out.append(records_for_linear(Wl[0][:, 3:]))                           # layer 0, feat part
    for l in SKIP_IN:
        out.append(records_for_linear(Wl[l][:, C + 3:]))                   # Z_l = W_l[:, feat] feat/sqrt2
    for l in range(1, MLP_LAYERS - 1):
        if l in SKIP_IN:
            out.append(records_for_linear(Wl[l][:, :C]))                   # x part
        else:
            out.append(records_for_linear(Wl[l]))
    recs = np.concatenate(out, axis=0)
    assert recs.shape == (G_TOTAL * 4, 64), recs.shape
    flat = _interleave(recs)
    out = np.concatenate([flat, np.zeros(RING * GROUP_FLOATS, np.float32)])
    assert out.size == REC_FLOATS
    return out


# ----------------------------------------------------------------------------- #
# small parameters ("row-param" order [tile][hi][r])
# ----------------------------------------------------------------------------- #
def rowparam(v):
    """feature vector [32*T] -> [T][hi][r] order (flattened)."""
    v = np.asarray(v, np.float32)
    T = v.shape[0] // 32
    idx = (32 * np.arange(T))[:, None, None] + ROW_TABLE[None, :, :]     # [T, 2, 16]
    return v[idx].reshape(-1)


def rowparam4(cols):
    """4 feature vectors [4][32*T] -> [T][hi][r][4] (one float4 per register)."""
    stacked = np.stack([rowparam(c).reshape(-1) for c in cols], axis=-1)
    return stacked.reshape(-1)


class ParamLayout(object):
    """Offsets (in floats) of every section of the params buffer; mirrored by the
    constants in csrc/sdf_layout.h."""

    def __init__(self):
        o = 0

        def take(n):
            nonlocal o
            s = o
            o += n
            return s
        self.PP = take(C * 4)                      # point_proj (w0, w1, w2, b)
        self.blk = []
        for _ in range(BLOCKS):
            d = {}
            d["ln1_g"] = take(C)
            d["ln1_b"] = take(C)
            d["bproj"] = take(C)
            d["bqkv"] = take(HEADS * 3 * 32)       # [head][q,k,v][hi][r]
            d["ln2_g"] = take(C)
            d["ln2_b"] = take(C)
            d["b2"] = take(C)
            d["b1"] = take(HID)
            self.blk.append(d)
        self.lnf_g = take(C)
        self.lnf_b = take(C)
        self.impl = []
        for l in range(MLP_LAYERS - 1):
            if l == 0 or l in SKIP_IN:
                self.impl.append(take(C * 4))      # (w_x, w_y, w_z, bias) per feature
            else:
                self.impl.append(take(C))          # bias
        self.w8 = take(C)
        self.b8 = take(16)
        self.total = o


PARAMS = ParamLayout()
assert PARAMS.total <= PARAM_FLOATS
P_FLAG = 13600   # split program only: uint32, non-zero = an operand outside the fp16 range (or not finite)
P_KMAX = 13616   # split program only: [BLOCKS][HEADS] largest |k_l| over the latent rows of the image
assert PARAMS.total <= P_FLAG and P_FLAG + 4 <= P_KMAX and P_KMAX + BLOCKS * HEADS <= PARAM_FLOATS
BLOCK_PARAM_FLOATS = 3 * C + HEADS * 96 + 3 * C + HID


def pack_params(sd):
    g = lambda k: np.asarray(sd[k], np.float32)
    out = np.zeros(PARAM_FLOATS, np.float32)

    def put(off, arr):
        out[off:off + arr.size] = arr
    Wp = g("point_proj.proj.weight")
    put(PARAMS.PP, rowparam4([Wp[:, 0], Wp[:, 1], Wp[:, 2], g("point_proj.proj.bias")]))
    for blk in range(BLOCKS):
        p, d = "blocks_attn.%d." % blk, PARAMS.blk[blk]
        put(d["ln1_g"], rowparam(g(p + "norm1.weight")))
        put(d["ln1_b"], rowparam(g(p + "norm1.bias")))
        put(d["bproj"], rowparam(g(p + "attn.proj.bias")))
        bq = g(p + "attn.qkv.bias")
        parts = []
        for h in range(HEADS):
            for part in range(3):
                parts.append(rowparam(bq[part * C + h * HD: part * C + (h + 1) * HD]))
        put(d["bqkv"], np.concatenate(parts))
        put(d["ln2_g"], rowparam(g(p + "norm2.weight")))
        put(d["ln2_b"], rowparam(g(p + "norm2.bias")))
        put(d["b2"], rowparam(g(p + "mlp.fc2.bias")))
        put(d["b1"], rowparam(g(p + "mlp.fc1.bias")))
    put(PARAMS.lnf_g, rowparam(g("norm.weight")))
    put(PARAMS.lnf_b, rowparam(g("norm.bias")))
    for l in range(MLP_LAYERS - 1):
        W, b = g("impl_mlp.layers.%d.weight" % l), g("impl_mlp.layers.%d.bias" % l)
        if l == 0:
            put(PARAMS.impl[l], rowparam4([W[:, 0], W[:, 1], W[:, 2], b]))
        elif l in SKIP_IN:
            put(PARAMS.impl[l], rowparam4([W[:, C], W[:, C + 1], W[:, C + 2], b]))
        else:
            put(PARAMS.impl[l], rowparam(b))
    put(PARAMS.w8, rowparam(g("impl_mlp.layers.8.weight")[0]))
    out[PARAMS.b8] = g("impl_mlp.layers.8.bias")[0]
    return out


def pack_program(sd, kv=None):
    """One decoder program: [record stream | params] (PROGRAM_FLOATS fp32)."""
    out = np.concatenate([pack_records(sd, kv), pack_params(sd)])
    assert out.size == PROGRAM_FLOATS
    return out


# ----------------------------------------------------------------------------- #
# latent-path parameters for the prologue kernels (weights transposed to [K][N])
# ----------------------------------------------------------------------------- #
class LatentLayout(object):
    def __init__(self, latent_dim=C):
        o = 0

        def take(n):
            nonlocal o
            s = o
            o += n
            return s
        self.latent_dim = latent_dim
        self.Wlp = take(latent_dim * C)
        self.blp = take(C)
        self.pos = take(L * C)
        self.ln1g0 = take(C)
        self.ln1b0 = take(C)
        self.Wqkv0 = take(C * 3 * C)
        self.bqkv0 = take(3 * C)
        self.Wproj0 = take(C * C)
        self.bproj0 = take(C)
        self.ln2g0 = take(C)
        self.ln2b0 = take(C)
        self.W1 = take(C * HID)
        self.b1 = take(HID)
        self.W2 = take(HID * C)
        self.b2 = take(C)
        self.ln1g1 = take(C)
        self.ln1b1 = take(C)
        self.Wkv1 = take(C * 2 * C)
        self.bkv1 = take(2 * C)
        self.total = o


LATENT = LatentLayout()


def pack_latent_params(sd):
    g = lambda k: np.asarray(sd[k], np.float32)
    assert g("latent_proj.weight").shape == (C, LATENT.latent_dim)
    out = np.zeros(LATENT.total, np.float32)

    def put(off, arr):
        arr = np.ascontiguousarray(arr, np.float32).reshape(-1)
        out[off:off + arr.size] = arr
    put(LATENT.Wlp, g("latent_proj.weight").T)
    put(LATENT.blp, g("latent_proj.bias"))
    put(LATENT.pos, g("pos_embed").reshape(L, C))
    b0, b1 = "blocks_attn.0.", "blocks_attn.1."
    put(LATENT.ln1g0, g(b0 + "norm1.weight"))
    put(LATENT.ln1b0, g(b0 + "norm1.bias"))
    put(LATENT.Wqkv0, g(b0 + "attn.qkv.weight").T)
    put(LATENT.bqkv0, g(b0 + "attn.qkv.bias"))
    put(LATENT.Wproj0, g(b0 + "attn.proj.weight").T)
    put(LATENT.bproj0, g(b0 + "attn.proj.bias"))
    put(LATENT.ln2g0, g(b0 + "norm2.weight"))
    put(LATENT.ln2b0, g(b0 + "norm2.bias"))
    put(LATENT.W1, g(b0 + "mlp.fc1.weight").T)
    put(LATENT.b1, g(b0 + "mlp.fc1.bias"))
    put(LATENT.W2, g(b0 + "mlp.fc2.weight").T)
    put(LATENT.b2, g(b0 + "mlp.fc2.bias"))
    put(LATENT.ln1g1, g(b1 + "norm1.weight"))
    put(LATENT.ln1b1, g(b1 + "norm1.bias"))
    put(LATENT.Wkv1, g(b1 + "attn.qkv.weight")[C:].T)     # k and v rows only
    put(LATENT.bkv1, g(b1 + "attn.qkv.bias")[C:])
    return out


# prologue scratch per image (floats): lat, x1, x2 [197x256]; qkv0 [197x768]; attn [197x256];
# hid [197x1024]; kv1 [197x512]
LPAD = 200  # rows padded to a multiple of the prologue's row block (4)
SCRATCH_FLOATS = LPAD * (3 * C + 3 * C + C + HID + 2 * C)


# ----------------------------------------------------------------------------- #
# split-fp16 program (csrc/sdf_decoder_split.hip) - host mirror of zs_sdf_split_programs
# ----------------------------------------------------------------------------- #
# One K-block (K = 16, three fp16 MFMAs) = two fp32 groups = records 8j..8j+7 of a 32x32 weight
# unit; per lane [hi: 8 fp16][lo: 8 fp16] with x ~= hi + lo (both rounded to nearest even).  Same units and byte size as the fp32
# program; the product derives it on the device, this mirror exists for tests and documentation.
KB_TOTAL = G_TOTAL // 2                 # 4,928 K-blocks per wave tile
KB_WORDS = 512                          # 32-bit words per K-block (2 x 64 lanes x 16 B)


def split_source_kblocks(n=None):
    """dst K-block -> src K-block (in fp32-program order).  Identity except inside the two MLP
    sections, where the kernel runs a software pipeline over the 32 hidden tiles (fc1 of tile
    t+1 before fc2 of tile t): fc1(0), [fc1(1), fc2(0)], ..., [fc1(31), fc2(30)], fc2(31), and in
    impl_mlp, where the skip layers contract their feat halves in place."""
    n = REC_FLOATS // GROUP_FLOATS // 2 if n is None else n
    src = np.arange(n)
    kb_block, kb_att = G_BLOCK // 2, HEADS * G_HEAD // 2
    order = list(range(16))
    for t in range(HT - 1):
        order += [(t + 1) * 32 + r for r in range(16)] + [t * 32 + 16 + r for r in range(16)]
    order += [(HT - 1) * 32 + 16 + r for r in range(16)]
    assert sorted(order) == list(range(HT * 32))
    for blk in range(BLOCKS):
        base = blk * kb_block + kb_att
        src[base:base + HT * 32] = base + np.array(order)
    # impl_mlp.  fp32 program: L0 | Z2 Z4 Z6 (feat halves of the skip layers) | L1 | L2x L3 | L4x L5 | L6x L7;
    # split stream: L0 | L1 | per pair: for each output tile [x part | feat part] (16 + 16 K-blocks), plain layer
    b0, kl = BLOCKS * kb_block, NT * NT * 2
    impl = list(range(kl)) + [4 * kl + i for i in range(kl)]
    for pair in range(3):
        for nt in range(NT):
            impl += [(5 + 2 * pair) * kl + nt * 2 * NT + w for w in range(2 * NT)]
            impl += [(1 + pair) * kl + nt * 2 * NT + w for w in range(2 * NT)]
        impl += [(6 + 2 * pair) * kl + i for i in range(kl)]
    assert sorted(impl) == list(range(G_IMPL // 2))
    src[b0:b0 + G_IMPL // 2] = b0 + np.array(impl)
    return src


def f16_round(x):
    """fp32 -> fp16 rounded to nearest even, overflowing to +-inf from 65520 (v_cvt_pk_f16_f32):
    (uint16 bits, value as fp32)."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    return h.view(np.uint16), h.astype(np.float32)


def f16_rtz(x):
    """fp32 -> fp16 rounded toward zero, saturating at +-65504 (v_cvt_pkrtz_f16_f32) - the rounding of
    rounds 1-2, kept for the A/B comparison in tests/test_program_packing.py."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    away = np.abs(h.astype(np.float32)) > np.abs(x)          # rounded away from zero (or to inf)
    h = np.where(away, np.nextafter(h, np.float16(0)), h).astype(np.float16)
    return h.view(np.uint16), h.astype(np.float32)


def split_program(prog):
    """fp32 program [PROGRAM_FLOATS] (float32) -> split program as uint32 words, bit for bit
    what zs_sdf_split_programs writes."""
    prog = np.ascontiguousarray(prog, np.float32)
    rec = prog[:REC_FLOATS].reshape(-1, 2, 64, 4)                  # [kb][group][lane][j]
    rec = rec[split_source_kblocks(rec.shape[0])]
    vals = rec.transpose(0, 2, 1, 3).reshape(-1, 64, 8)             # [kb][lane][e = 4 g + j]
    hi16, hif = f16_round(vals)
    with np.errstate(invalid="ignore"):
        lo16, _ = f16_round(vals - hif)
    out = np.stack([hi16, lo16], axis=1)                            # [kb][hi | lo][lane][8]
    words = np.ascontiguousarray(out).reshape(-1).view(np.uint32)
    params = prog[REC_FLOATS:].copy()
    params[P_KMAX:P_KMAX + BLOCKS * HEADS] = latent_k_bounds(prog).reshape(-1)
    bad = not (np.all(np.isfinite(prog)) and float(np.abs(prog).max()) <= F16_MAX)
    params[P_FLAG:P_FLAG + 1].view(np.uint32)[0] = 1 if bad else 0
    return np.concatenate([words, params.view(np.uint32)])


# ----------------------------------------------------------------------------- #
# tested envelope of the split-fp16 arithmetic (tests/test_gpu_decoder_split.py)
# ----------------------------------------------------------------------------- #
# The 2^-21 operand error of the split acts on the attention logits in absolute terms:
# |dS| <= 2.5 * 2^-21 * scale * |q| |k|.  Measured against the exact-fp32 kernel: 3.4e-6 on the
# seeded weights (scale |q||k| ~ 5), 2e-5 with the attention weights x4, 3e-4 at x10.  The contract
# is 1e-4 on the logits, so:
#   * on the DEVICE, every 128-point tile whose points reach  scale * |q_h| * max_l |k_h,l| > S_GUARD
#     in any head, or whose program holds an operand that is not finite / outside the fp16 range, is
#     flagged by the split kernel and re-evaluated by the exact-fp32 kernel (same stream, no host
#     round trip: Implicit.query_* enqueue both launches);
#   * on the HOST, weights beyond W_MAX (hidden activations could leave the fp16 range) select the
#     exact-fp32 kernels for the whole call (Implicit.prepare).
S_GUARD = 64.0
W_MAX = 16.0
F16_MAX = 65504.0


def split_envelope(sd):
    """(inside, report) for the weights alone: finite and |w| <= W_MAX."""
    vals = [np.asarray(v, np.float32) for k, v in sd.items() if k != "pos_embed"]
    wmax = max(float(np.max(np.abs(v))) if np.all(np.isfinite(v)) else float("inf") for v in vals)
    return wmax <= W_MAX, dict(max_abs_weight=wmax)


def latent_k_bounds(prog):
    """[BLOCKS, HEADS] largest |k_l| over the latent rows, from the K records of one fp32 program
    (host mirror of what zs_sdf_split_programs writes at P_KMAX)."""
    prog = np.ascontiguousarray(prog, np.float32)
    out = np.zeros((BLOCKS, HEADS), np.float32)
    for blk in range(BLOCKS):
        for h in range(HEADS):
            o = kv_group_offset(blk, h) * GROUP_FLOATS
            g = prog[o:o + G_KV_HEAD * GROUP_FLOATS].reshape(LT, 8, 64, 4)[:, :4]      # K groups of every tile
            rec = g.transpose(0, 1, 3, 2).reshape(LT, 16, 64)                          # [lt][r][lane]
            sq = (rec.astype(np.float64) ** 2).sum(1)                                  # over r: half the dims per lane
            row = sq[:, :32] + sq[:, 32:]                                              # lanes l, l + 32: the two halves
            out[blk, h] = np.sqrt(row.max())
    return out


# ----------------------------------------------------------------------------- #
# block 0's point-side q/k/v as a rank-4 table (csrc/sdf_decoder_split.hip: block0_window_kernel)
# ----------------------------------------------------------------------------- #
# Block 0's point row is pf = point_proj(xyz) = A p~, p~ = (x, y, z, 1), so LN1(pf) = rstd * g (A - 1 m) p~ + b with m the
# column mean of A and rstd the per-point scalar, and for the 768 rows of block 0's qkv
#     qkv = rstd * (T p~) + c,    T = Wqkv diag(g) (A - 1 m)  [768 x 4],    c = Wqkv b + bqkv.
# T and c go into a 4,096-float window per image.  The split kernel no longer reads it directly: block0_stream_kernel builds
# the compact block-0 stream (below) from it, and a launch whose streams do not fit runs block 0's three 256 -> 256 GEMMs per
# head from the program, like block 1 (the program keeps all its K-blocks either way).
B0_WINDOW_FLOATS = 4096
B0_BPROJ, B0_C, B0_T = 0, C, C + HEADS * 96      # [b_proj 256][c 768: row-param order][T 3072: [tile][hi][r][4]]
KB_HEAD = G_HEAD // 2                            # 92 K-blocks per head: 48 q/k/v, 28 latent K/V, 16 proj
KB_QKV_HEAD = G_QKV_HEAD // 2                    # 48


def _kblock_values(words, kb):
    """K-block `kb` of a split program (uint32 words) as float64 [lane][8]: hi + lo."""
    h = np.ascontiguousarray(words[kb * KB_WORDS:(kb + 1) * KB_WORDS]).view(np.float16).reshape(2, 64, 8)
    return h[0].astype(np.float64) + h[1].astype(np.float64)


def block0_qkv_weights(split_prog):
    """Block 0's qkv weight [768, 256] (rows in the order of attn.qkv.weight) as the split program holds it: hi + lo, float64."""
    W = np.zeros((3 * C, C), np.float64)
    for h in range(HEADS):
        for part in range(3):
            for kt in range(NT):
                for j in range(2):
                    v = _kblock_values(split_prog, h * KB_HEAD + part * 2 * NT + kt * 2 + j)       # [lane][e]: record 8 j + e
                    rows = part * C + h * HD + LANE_I                                              # [64]
                    cols = 32 * kt + ROW_TABLE[LANE_HI][:, 8 * j:8 * j + 8]                        # [64, 8]
                    W[rows[:, None], cols] = v
    return W


def _from_rowparam(v):
    """Inverse of rowparam: [T][hi][r] order -> feature order."""
    v = np.asarray(v)
    T = v.shape[0] // 32
    idx = ((32 * np.arange(T))[:, None, None] + ROW_TABLE[None, :, :]).reshape(-1)
    out = np.empty_like(v)
    out[idx] = v
    return out


def block0_window(split_prog):
    """The 4,096 floats that stand for block 0's LN1 / q, k, v GEMMs (the compact stream's q, k, v and U operands are built
    from them), from one SPLIT program (uint32 words, split_program()): [b_proj | c | T] as laid out above, computed in
    float64 and rounded once to float32 - host mirror of zs_sdf_block0_tables."""
    words = np.ascontiguousarray(split_prog).view(np.uint32)
    params = words[REC_FLOATS:].view(np.float32).astype(np.float64)
    d = PARAMS.blk[0]
    A = np.stack([_from_rowparam(params[PARAMS.PP + i:PARAMS.PP + 4 * C:4]) for i in range(4)], axis=1)   # [256, 4]: w0 w1 w2 b
    g = _from_rowparam(params[d["ln1_g"]:d["ln1_g"] + C])
    b = _from_rowparam(params[d["ln1_b"]:d["ln1_b"] + C])
    W = block0_qkv_weights(words)
    T = W @ (g[:, None] * (A - A.mean(axis=0, keepdims=True)))                                       # [768, 4]
    c = W @ b                                                                                         # + bqkv below (row-param)
    out = np.zeros(B0_WINDOW_FLOATS, np.float64)
    out[B0_BPROJ:B0_BPROJ + C] = params[d["bproj"]:d["bproj"] + C]
    for h in range(HEADS):
        for part in range(3):
            tile = 3 * h + part
            rows = slice(part * C + h * HD, part * C + (h + 1) * HD)
            out[B0_C + tile * 32:B0_C + (tile + 1) * 32] = \
                _rowparam64(c[rows]) + params[d["bqkv"] + tile * 32:d["bqkv"] + (tile + 1) * 32]
            out[B0_T + tile * 128:B0_T + (tile + 1) * 128] = \
                np.stack([_rowparam64(T[rows, i]) for i in range(4)], axis=-1).reshape(-1)
    return out.astype(np.float32)


def _rowparam64(v):
    """rowparam without the float32 rounding."""
    v = np.asarray(v, np.float64)
    T = v.shape[0] // 32
    idx = (32 * np.arange(T))[:, None, None] + ROW_TABLE[None, :, :]
    return v[idx].reshape(-1)


# ----------------------------------------------------------------------------- #
# block 0 from a compact stream of its own (csrc/sdf_decoder_split.hip: block0_stream_kernel, BLOCK 0 STREAM)
# ----------------------------------------------------------------------------- #
# With the table, q_h = rstd (T_q p~) + c_q is affine in u = (rstd x, rstd y, rstd z, rstd, 1), so the 224 latent logits of a
# head are S_h = U_h u with U_h = c K_h [T_q,h | c_q,h] (224 x 5; K_h the image's K rows, c = 32^-1/2 log2 e folded in), and
# q, k, v themselves are [T | c] u.  A rank-5 contraction with both operands split needs 15 products per output
# (U_hi u_hi + U_hi u_lo + U_lo u_hi): the K = 16 of ONE v_mfma_f32_32x32x16_f16.  Lane l of an operand holds k = 8 (l >> 5) + e:
#     A (32 rows x 16, one 1 KiB half of a K-block slot)   lanes  0-31: [Uh0 Uh1 Uh2 Uh3 | Ud0 Ud1 Ud2 Ud3]
#                                                            lanes 32-63: [Ul0 Ul1 Ul2 Ul3 | Uh4 Ud4 Ul4 0]
#     B (16 x 32 points, the same for every A of a tile)     lanes  0-31: [uh0 uh1 uh2 uh3 | ul0 ul1 ul2 ul3]
#                                                            lanes 32-63: [ud0 ud1 ud2 ud3 | uh4 ul4 ud4 0]
# with xh = fp16(x), xl = fp16(s (x - xh)), xd = fp16(xh / s), s = B0S_LO_SCALE: the remainders of values of order 0.1 .. 1 are
# of order 1e-5 .. 1e-4, where fp16 is subnormal (spacing 6e-8, an ABSOLUTE error that the other operand multiplies by up to
# ~10); scaled by s = 64 before the rounding they keep their 11 bits, and the power of two is taken back exactly by the hi
# copy that meets them (xd is inexact only where xh / s is itself subnormal - an error the small remainder multiplies).
# Block 0 then needs, per head, 10 packed operands (q, k, v, U_0..U_6) = 5 K-block slots [a | b] (a in the hi half, b in the
# lo half), the 13 V K-blocks whose probabilities can be non-zero (the second K-block of latent tile 6 multiplies rows
# 208-223, which are masked) and the 16 proj K-blocks: 34 slots, 97 MFMAs.  They are written per image in consumption order
# into a stream of 8 x 34 = 272 slots = 34 whole chunks; behind it the kernel continues in the program at K-block 736.
B0S_KB_HEAD = 34
B0S_KB = HEADS * B0S_KB_HEAD                     # 272 K-block slots
B0S_WORDS = B0S_KB * KB_WORDS                    # 544 KiB per image
B0S_OPERANDS = 3 + LT                            # q, k, v, U_0 .. U_6
SPLIT_MFMAS_B0_STREAM = HEADS * (B0S_OPERANDS + 3 * (2 * LT - 1 + 2 * NT)) + 3 * (KB_TOTAL - HEADS * KB_HEAD)   # 13,352
SLAB_REGION_BYTES = 256 * 4 * (3 * NT * 4 * 64) * 16   # csrc/sdf_query.h: the workspace's slab region (96 MiB)
LOG2E = 1.44269504088896340736
B0S_LO_SCALE = 64.0


def block0_stream_slots():
    """The 34 slots of one head in consumption order: ("pack", a, b) = packed operands a | b (0 q, 1 k, 2 v, 3 + lt: U_lt),
    ("copy", kb) = K-block kb of the head's 92 in the split program (V of latent tile lt: 48 + 4 lt + 2 + j; proj: 76 + i)."""
    v = lambda lt, n=2: [("copy", KB_QKV_HEAD + 4 * lt + 2 + j) for j in range(n)]
    slots = [("pack", 0, 1), ("pack", 2, 3)] + v(0)
    for lt in (1, 3, 5):
        slots += [("pack", 3 + lt, 4 + lt)] + v(lt) + v(lt + 1, 2 if lt + 1 < LT - 1 else 1)
    slots += [("copy", KB_HEAD - 2 * NT + i) for i in range(2 * NT)]
    assert len(slots) == B0S_KB_HEAD
    return slots


def block0_stream_fit(batch):
    """Do the tables AND the compact streams of `batch` images fit the head of the workspace (csrc/sdf_query.h: 175 images)?
    A launch of more images runs block 0's q/k/v GEMMs from the program, as ZS_SPLIT_BLOCK0_GEMM=1 does."""
    return batch * (B0_WINDOW_FLOATS * 4 + B0S_WORDS * 4) <= SLAB_REGION_BYTES


def block0_rank5_rows(split_prog, window=None):
    """[HEADS][10][32][5] float32: the rows (in A-row order: feature of the head / latent of the tile) of the ten rank-5
    operands of every head.  q, k, v: [T | c] straight from the table window; U_lt = c K_lt [T_q | c_q], summed in float64
    over the head's 32 features in order, from hi + lo of the split program's K records, rounded once to float32."""
    words = np.ascontiguousarray(split_prog).view(np.uint32)
    window = block0_window(words) if window is None else np.asarray(window, np.float32)
    out = np.zeros((HEADS, B0S_OPERANDS, 32, 5), np.float32)
    inv = np.empty(32, np.int64)
    inv[ROW_TABLE.reshape(-1)] = np.arange(32)                  # feature t sits at row-param position inv[t] = hh * 16 + r
    for h in range(HEADS):
        for part in range(3):
            tile = 3 * h + part
            out[h, part, :, :4] = window[B0_T + tile * 128:B0_T + (tile + 1) * 128].reshape(32, 4)[inv]
            out[h, part, :, 4] = window[B0_C + tile * 32:B0_C + (tile + 1) * 32][inv]
        uq = out[h, 0].astype(np.float64)                       # [32 features][5]
        for lt in range(LT):
            K = np.zeros((32, HD), np.float64)
            for j in range(2):
                v = _kblock_values(words, h * KB_HEAD + KB_QKV_HEAD + 4 * lt + j)     # [lane][e]: K[row][row(8 j + e, hi)]
                K[LANE_I[:, None], ROW_TABLE[LANE_HI][:, 8 * j:8 * j + 8]] = v
            acc = np.zeros((32, 5), np.float64)
            for f in range(HD):
                acc += K[:, f:f + 1] * uq[f][None, :]
            out[h, 3 + lt] = (acc * (HD ** -0.5 * LOG2E)).astype(np.float32)
    return out


def _split_scaled(x):
    """x float32 -> fp16 bit patterns of (hi, hi / s, s lo): hi = fp16(x), lo = x - hi scaled by s = B0S_LO_SCALE BEFORE it is
    rounded to fp16 (so that it stays out of fp16's subnormals), and the copy of hi that meets a scaled lo divided by s."""
    x = np.ascontiguousarray(x, np.float32)
    hb, hf = f16_round(x)
    with np.errstate(invalid="ignore"):
        lb, _ = f16_round((x - hf) * np.float32(B0S_LO_SCALE))
    db, _ = f16_round(hf * np.float32(1.0 / B0S_LO_SCALE))
    return hb, db, lb


def pack_rank5_a(rows):
    """[32][5] float32 -> the A operand [64 lanes][8] as fp16 bit patterns (uint16), layout above."""
    h, d, l = _split_scaled(rows)
    z = np.zeros(32, np.uint16)
    lo_lanes = np.stack([h[:, 0], h[:, 1], h[:, 2], h[:, 3], d[:, 0], d[:, 1], d[:, 2], d[:, 3]], axis=1)
    hi_lanes = np.stack([l[:, 0], l[:, 1], l[:, 2], l[:, 3], h[:, 4], d[:, 4], l[:, 4], z], axis=1)
    return np.concatenate([lo_lanes, hi_lanes], axis=0)


def pack_rank5_b(u):
    """u [32 points][5] float32 -> the B operand [64 lanes][8] as fp16 bit patterns (uint16), layout above."""
    h, d, l = _split_scaled(u)
    z = np.zeros(h.shape[0], np.uint16)
    lo_lanes = np.stack([h[:, 0], h[:, 1], h[:, 2], h[:, 3], l[:, 0], l[:, 1], l[:, 2], l[:, 3]], axis=1)
    hi_lanes = np.stack([d[:, 0], d[:, 1], d[:, 2], d[:, 3], h[:, 4], l[:, 4], d[:, 4], z], axis=1)
    return np.concatenate([lo_lanes, hi_lanes], axis=0)


def block0_stream(split_prog, window=None):
    """The compact block-0 stream of one SPLIT program as uint32 words [B0S_WORDS] - host mirror of zs_sdf_block0_streams."""
    words = np.ascontiguousarray(split_prog).view(np.uint32)
    rows = block0_rank5_rows(words, window)
    out = np.zeros((B0S_KB, KB_WORDS), np.uint32)
    for h in range(HEADS):
        for i, slot in enumerate(block0_stream_slots()):
            dst = out[h * B0S_KB_HEAD + i]
            if slot[0] == "copy":
                kb = h * KB_HEAD + slot[1]
                dst[:] = words[kb * KB_WORDS:(kb + 1) * KB_WORDS]
            else:
                for half, op in enumerate(slot[1:]):
                    dst[half * 256:(half + 1) * 256] = np.ascontiguousarray(pack_rank5_a(rows[h, op])).reshape(-1).view(np.uint32)
    return out.reshape(-1)


def split_consumed_slots_b0_stream():
    """What the weight stream delivers when block 0 runs from its compact stream: ("b0", i) for i = 0..271, then ("prog", kb)
    for the split program's K-blocks 736 on - 4,464 slots per wave tile."""
    return [("b0", i) for i in range(B0S_KB)] + [("prog", kb) for kb in range(HEADS * KB_HEAD, KB_TOTAL)]
