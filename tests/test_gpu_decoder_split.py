"""GPU parity of the split-fp16 ("f16x3") decoder (csrc/sdf_decoder_split.hip, through the C
ABI) against the oracle, the goldens of the real reference and the exact-fp32 kernel.

Bar (BASELINE.json north_star): logits / occupancy within 1e-4 absolute.  Split-fp16 carries
~2^-21 relative operand error through ~25 dependent stages: measured max |logit difference| to
the fp32 kernel 3.4e-6 on the 129^3 grid (no occupancy flip); asserted at 1.5e-5.  Occupancy
indices (occ > 0.5) must agree outside |logit| < BAND."""
import numpy as np
import pytest
import torch

from oracle import decoder_ref as R
from zeroshape_amd import program as P
from zeroshape_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ATOL = 1.5e-5   # contract 1e-4
BAND = 1e-5     # |logit| below which an occupancy flip is inside the arithmetic's error


@pytest.fixture(scope="module")
def net(seeded_sd):
    from zeroshape_amd.model.shape.implicit import Implicit
    m = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                 n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                 posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    m.load_state_dict(seeded_sd, strict=True)
    m = m.cuda().eval()
    m.precision = "f16x3"
    return m


def test_split_program_layout(net, seeded_sd):
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2)).cuda()
    f32 = net.prepare(latent, "f32")
    sp = net.prepare(latent, "f16x3")
    assert sp.precision == "f16x3" and sp.programs.shape == f32.programs.shape
    assert sp.exact is not None and torch.equal(sp.exact, f32.programs)
    km = slice(P.REC_FLOATS + P.P_KMAX, P.REC_FLOATS + P.P_KMAX + P.BLOCKS * P.HEADS)
    for b in range(2):
        want = P.split_program(f32.programs[b].cpu().numpy())
        got = sp.programs[b].cpu().numpy().view(np.uint32)
        # the K-norm bounds of the envelope guard are fp32 sums on the device, fp64 in the mirror
        np.testing.assert_allclose(got[km].view(np.float32), want[km].view(np.float32), rtol=1e-6)
        assert 0.5 < float(got[km].view(np.float32).min())
        got[km], want[km] = 0, 0
        np.testing.assert_array_equal(got, want)
        assert got[P.REC_FLOATS + P.P_FLAG] == 0


@pytest.mark.parametrize("m", [1, 31, 32, 33, 127, 128, 129, 1000])
def test_ragged_point_counts_vs_oracle(net, seeded_sd, m):
    latent = torch.from_numpy(syn.seeded_latent(seed=3, batch=1))
    pts = torch.from_numpy(syn.seeded_cloud(m, 1, m, -1.5, 1.5))
    want, _ = R.implicit_forward(seeded_sd, latent, pts)
    got, attn = net(latent.cuda(), None, pts.cuda(), need_attn=False)
    assert attn is None
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=ATOL, rtol=0)


def test_training_shape_points_vs_golden_and_fp32_kernel(net, decoder_golden):
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2)).cuda()
    rs = np.random.RandomState(123)
    pts = torch.from_numpy(rs.uniform(-1, 1, size=(2, 4096, 3)).astype(np.float32)).cuda()
    lg, _ = net(latent, None, pts, need_attn=False)
    np.testing.assert_allclose(lg.cpu().numpy(), decoder_golden["pts4096_logit"], atol=ATOL, rtol=0)
    exact = net.query_points(net.prepare(latent, "f32"), pts)
    err = (lg - exact).abs()
    assert float(err.max()) < ATOL and float(err.mean()) < 2e-6
    # the reference's default call (with the attention map): the map comes from the fp32 kernel,
    # the logits are the same numbers as without it
    lg2, attn = net(latent, None, pts)
    assert torch.equal(lg2, lg) and attn.shape == (2, 4096, 197)
    np.testing.assert_allclose(attn[:, ::512].cpu().numpy(), decoder_golden["pts4096_attn_rows"], atol=2e-7, rtol=0)
    assert int(net.last_tile_flags.sum()) == 0            # the seeded network is inside the envelope


def test_grid32_full_vs_golden(net, decoder_golden):
    from zeroshape_amd.utils import eval_3D as E
    from zeroshape_amd.utils.options import EasyDict as edict
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2))[:1].cuda()
    opt = edict(dict(device="cuda", H=224, W=224, eval=dict(vox_res=32, range=[-1.5, 1.5]),
                     arch=dict(win_size=16)))
    var = edict(dict(idx=[0]))
    grid = E.get_dense_3D_grid(opt, var)
    occ, _ = E.compute_level_grid(opt, net, latent, None, grid, None, vis_attn=False)
    occ = occ[0].cpu().numpy()
    np.testing.assert_allclose(occ[::5, ::5, ::5], decoder_golden["occ32_stride5"], atol=ATOL, rtol=0)
    bits = np.unpackbits(decoder_golden["occ32_bits"])[: occ.size].astype(bool)
    lg = net.query_grid(latent, grid._zs_grid.axis, apply_sigmoid=False)[0].cpu().numpy()
    mism = (occ > 0.5).reshape(-1) != bits
    assert np.all(np.abs(lg.reshape(-1)[mism]) < BAND), "occupancy flip outside the error band"
    assert mism.sum() <= 2
    for i in (0, 16, 32):
        np.testing.assert_allclose(lg[i].reshape(-1), decoder_golden["logit32_slice%d" % i], atol=ATOL, rtol=0)


def test_full_size_grid128_properties(net, seeded_sd):
    """129^3 points: slab decomposition exact (multi-GPU sharding), 2048 random grid points
    against the oracle, agreement with the fp32 kernel on a slab."""
    N = 128
    latent_c = torch.from_numpy(syn.seeded_latent(seed=0, batch=1))
    latent = latent_c.cuda()
    axis = torch.linspace(-1.5, 1.5, N + 1, device="cuda")
    st = net.prepare(latent)
    full = net.query_grid(latent, axis, apply_sigmoid=False, state=st)
    assert full.shape == (1, N + 1, N + 1, N + 1)
    slab = net.query_grid(latent, axis, apply_sigmoid=False, slice_begin=40, slice_end=57, state=st)
    assert torch.equal(full[:, 40:57], slab)
    exact = net.query_grid(latent, axis, apply_sigmoid=False, slice_begin=40, slice_end=57,
                           state=net.prepare(latent, "f32"))
    err = (slab - exact).abs()
    assert float(err.max()) < ATOL
    flips = (slab > 0) != (exact > 0)
    assert bool(torch.all(exact[flips].abs() < BAND))
    rs = np.random.RandomState(7)
    idx = rs.randint(0, N + 1, size=(2048, 3))
    ax = axis.cpu()
    pts = torch.stack([ax[idx[:, 0]], ax[idx[:, 1]], ax[idx[:, 2]]], -1)[None]
    want, _ = R.implicit_forward(seeded_sd, latent_c, pts)
    got = full[0, idx[:, 0], idx[:, 1], idx[:, 2]].cpu().numpy()
    np.testing.assert_allclose(got, want[0].numpy(), atol=ATOL, rtol=0)
    # repeatable: the same launch twice is bit-identical (no race in the staged weight stream)
    again = net.query_grid(latent, axis, apply_sigmoid=False, state=st)
    assert torch.equal(full, again)


def test_batched_grid_equals_per_image(net):
    latent = torch.from_numpy(syn.seeded_latent(seed=2, batch=2)).cuda()
    axis = torch.linspace(-1.5, 1.5, 33, device="cuda")
    both = net.query_grid(latent, axis, apply_sigmoid=True)
    one = net.query_grid(latent[1:], axis, apply_sigmoid=True)
    assert torch.equal(both[1:], one)


def test_bad_precision_raises(net):
    with pytest.raises(ValueError):
        net.prepare(torch.zeros(1, 197, 256).cuda(), "fp8")
    st = net.prepare(torch.zeros(1, 197, 256).cuda(), "f16x3")
    with pytest.raises(ValueError):
        net.query_points(st, torch.zeros(1, 4, 3).cuda(), need_attn=True)


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_point_range_query_equals_grid(net, prec):
    """zs_sdf_query_grid_range[_split]: any point range of the grid in memory order, bit for bit
    (the unit of the multi-GPU sharding), including ranges that start and end inside a tile."""
    latent = torch.from_numpy(syn.seeded_latent(seed=4, batch=2)).cuda()
    G = 33
    axis = torch.linspace(-1.5, 1.5, G, device="cuda")
    st = net.prepare(latent, prec)
    full = net.query_grid(latent, axis, apply_sigmoid=True, state=st).reshape(2, -1)
    for b, e in ((0, G ** 3), (0, 1), (1000, 1001), (4481, 17999), (G ** 3 - 77, G ** 3), (500, 500)):
        got = net.query_grid_range(latent, axis, b, e, apply_sigmoid=True, state=st)
        assert got.shape == (2, e - b) and torch.equal(got, full[:, b:e])
    from zeroshape_amd import _lib
    with pytest.raises(_lib.ZeroShapeHipError):
        net.query_grid_range(latent, axis, 10, G ** 3 + 1, state=st)


@pytest.mark.parametrize("seed,gain,tol", [(1, 1.0, 2e-5), (2, 4.0, 2e-5), (3, 10.0, 1e-3)])
def test_other_weights_and_scales_vs_fp32_kernel(seed, gain, tol):
    """Different seeded weights, with the attention and MLP weights scaled up (peaky softmax,
    activations in the hundreds): the split arithmetic stays within 2e-5 of the logit scale of the
    exact-fp32 kernel, and both stay within the contract of the oracle.  The operand error 2^-21
    acts on the attention logits in absolute terms, |S| 2^-20: at gain 10 (|S| ~ 500, one-hot
    attention, 100x the logits of the seeded network) the difference reaches 3e-4 - measured, and
    bounded here; fp32 evaluations in different summation orders disagree by as much there."""
    from zeroshape_amd.model.shape.implicit import Implicit
    from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed
    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(seed, pos_embed=pe).items()}
    for k in sd:
        if k.endswith("attn.qkv.weight") or k.endswith("mlp.fc1.weight") or k.endswith("latent_proj.weight"):
            sd[k] = sd[k] * gain
    m = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                 n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                 posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.envelope_guard = False        # this test measures the arithmetic itself, also outside its envelope
    latent = torch.from_numpy(syn.seeded_latent(seed=seed, batch=2))
    pts = torch.from_numpy(syn.seeded_cloud(seed + 50, 2, 1500, -1.5, 1.5))
    exact = m.query_points(m.prepare(latent.cuda(), "f32"), pts.cuda())
    split = m.query_points(m.prepare(latent.cuda(), "f16x3", calibrate=False), pts.cuda())
    assert bool(torch.isfinite(split).all())
    scale = max(1.0, float(exact.abs().max()))
    assert float((split - exact).abs().max()) < tol * scale
    want, _ = R.implicit_forward(sd, latent, pts)
    # (at gain 10 two fp32 evaluations with different summation orders - the exact-fp32 kernel and
    # the CPU oracle - already differ by 1.8e-4: the split arithmetic is not the limit there)
    assert float((exact.cpu() - want).abs().max()) < max(1e-4, tol) * scale
    assert float((split.cpu() - want).abs().max()) < max(1e-4, tol) * scale


# --------------------------------------------------------------------------------------------- #
# f16x3 on the larger goldens of the real reference (tests/golden/make_golden.py)
# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("N", [64, 128])
def test_grid_slices_vs_golden(net, decoder_golden, N):
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2))[:1].cuda()
    axis = torch.linspace(-1.5, 1.5, N + 1, device="cuda")
    st = net.prepare(latent)
    assert st.precision == "f16x3"
    for i in (0, N // 2, N):
        lg = net.query_grid(latent, axis, apply_sigmoid=False, slice_begin=i, slice_end=i + 1, state=st)
        got = lg[0, 0].reshape(-1)[::16].cpu().numpy()
        np.testing.assert_allclose(got, decoder_golden["logit%d_slice%d_s16" % (N, i)], atol=ATOL, rtol=0)
        assert int(net.last_tile_flags.sum()) == 0


def test_vox256_slab_and_batched_grid(net, seeded_sd):
    """BASELINE config 5 geometry (257^3, sharded): one rank's slab of a batch of 2 images against
    the oracle on random points; slab launches of a batch equal per-image launches."""
    N = 256
    latent_c = torch.from_numpy(syn.seeded_latent(seed=2, batch=2))
    latent = latent_c.cuda()
    axis = torch.linspace(-1.5, 1.5, N + 1, device="cuda")
    st = net.prepare(latent)
    slab = net.query_grid(latent, axis, apply_sigmoid=False, slice_begin=224, slice_end=226, state=st)
    assert slab.shape == (2, 2, N + 1, N + 1)
    one = net.query_grid(latent[1:], axis, apply_sigmoid=False, slice_begin=224, slice_end=226)
    assert torch.equal(slab[1:], one)
    rs = np.random.RandomState(5)
    jj, kk = rs.randint(0, N + 1, 500), rs.randint(0, N + 1, 500)
    ax = axis.cpu()
    pts = torch.stack([ax[225].expand(500), ax[jj], ax[kk]], -1)[None].repeat(2, 1, 1)
    want, _ = R.implicit_forward(seeded_sd, latent_c, pts)
    got = slab[:, 1, jj, kk].cpu().numpy()
    np.testing.assert_allclose(got, want.numpy(), atol=ATOL, rtol=0)


# --------------------------------------------------------------------------------------------- #
# envelope guard (program.py: S_GUARD, W_MAX)
# --------------------------------------------------------------------------------------------- #
def _scaled_net(seed, gain):
    from zeroshape_amd.model.shape.implicit import Implicit
    from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed
    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(seed, pos_embed=pe).items()}
    for k in sd:
        if k.endswith("attn.qkv.weight") or k.endswith("mlp.fc1.weight") or k.endswith("latent_proj.weight"):
            sd[k] = sd[k] * gain
    m = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                 n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                 posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sd


def test_guard_reevaluates_out_of_envelope_tiles_in_fp32():
    """Attention weights x10 (|q||k| d^-1/2 in the hundreds, where the raw split arithmetic is 3e-4
    off): the device guard flags those tiles and the exact kernel rewrites them - the guarded
    result equals the fp32 kernel there and the split kernel elsewhere."""
    m, sd = _scaled_net(3, 10.0)
    latent = torch.from_numpy(syn.seeded_latent(seed=3, batch=2)).cuda()
    pts = torch.from_numpy(syn.seeded_cloud(53, 2, 1500, -1.5, 1.5)).cuda()
    st = m.prepare(latent, calibrate=False)      # (the calibration would hand these weights to the fp32 kernels)
    assert st.precision == "f16x3"
    guarded = m.query_points(st, pts)
    flags = m.last_tile_flags.clone().view(2, -1).bool()
    assert flags.shape[1] == 12 and bool(flags.any())
    exact = m.query_points(m.prepare(latent, "f32"), pts)
    m.envelope_guard = False
    raw = m.query_points(st, pts)
    per_point = flags.repeat_interleave(128, dim=1)[:, :1500]
    assert torch.equal(guarded[per_point], exact[per_point])
    assert torch.equal(guarded[~per_point], raw[~per_point])
    # the flag is the documented bound: d^-1/2 |q| max_l |k_l| > S_GUARD for some head of some point
    lp = R.latent_path(sd, latent.cpu())
    kmax = torch.stack([lp["k%d" % b].norm(dim=-1).amax(-1) for b in range(2)], 1)          # [B, blk, head]
    got = st.programs[:, P.REC_FLOATS + P.P_KMAX: P.REC_FLOATS + P.P_KMAX + 16].view(2, 2, 8).cpu()
    np.testing.assert_allclose(got.numpy(), kmax.numpy(), rtol=2e-5)
    # the same network with the seeded scale stays entirely on the split kernel
    m1, _ = _scaled_net(3, 1.0)
    m1.query_points(m1.prepare(latent), pts)
    assert int(m1.last_tile_flags.sum()) == 0


def test_guard_grid_and_range_paths():
    m, _ = _scaled_net(2, 10.0)
    latent = torch.from_numpy(syn.seeded_latent(seed=2, batch=1)).cuda()
    axis = torch.linspace(-1.5, 1.5, 17, device="cuda")
    st = m.prepare(latent, calibrate=False)
    g = m.query_grid(latent, axis, apply_sigmoid=True, state=st)
    fl = m.last_tile_flags.clone().bool()
    r = m.query_grid_range(latent, axis, 0, 17 ** 3, apply_sigmoid=True, state=st)
    assert torch.equal(g.reshape(1, -1), r) and torch.equal(fl, m.last_tile_flags.bool()) and bool(fl.any())
    exact = m.query_grid(latent, axis, apply_sigmoid=True, state=m.prepare(latent, "f32")).reshape(-1)
    pp = fl.repeat_interleave(128)[: 17 ** 3]
    assert torch.equal(g.reshape(-1)[pp], exact[pp])


def test_non_finite_inputs_give_nan_like_the_reference(net):
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2)).cuda()
    pts = torch.from_numpy(syn.seeded_cloud(9, 2, 300, -1, 1)).cuda()
    bad = latent.clone()
    bad[1, 5, 7] = float("nan")
    st = net.prepare(bad)
    assert int(st.programs[1].view(torch.int32)[P.REC_FLOATS + P.P_FLAG]) != 0
    assert int(st.programs[0].view(torch.int32)[P.REC_FLOATS + P.P_FLAG]) == 0
    out = net.query_points(st, pts)
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[0]).all())
    good = net.query_points(net.prepare(latent), pts)
    assert torch.equal(out[0], good[0])
    # a non-finite query coordinate poisons that point only
    p2 = pts.clone()
    p2[0, 17, 1] = float("inf")
    out2 = net.query_points(net.prepare(latent), p2)
    assert bool(torch.isnan(out2[0, 17])) and int(torch.isnan(out2).sum()) == 1
    for prec_guard in (True, False):
        net.envelope_guard = prec_guard
        o = net.query_points(net.prepare(bad), pts)
        assert bool(torch.isnan(o[1]).all())
    net.envelope_guard = True


def test_calibration_hands_out_of_contract_weights_to_the_exact_kernels():
    """Implicit.prepare measures the output error of the split arithmetic once per weight version (4096 probe
    points through both kernels) and keeps "f16x3" only within CALIBRATION_TOL: the seeded network stays, the
    same network with its attention weights x10 (raw error 3e-4) is evaluated by the fp32 kernels, and a non-finite
    first image does not poison the verdict."""
    latent = torch.from_numpy(syn.seeded_latent(seed=3, batch=1)).cuda()
    m1, _ = _scaled_net(3, 1.0)
    assert m1.prepare(latent).precision == "f16x3"
    c1 = m1.last_calibration
    assert c1["selected"] == "f16x3" and 0 < c1["max_abs_diff"] <= m1.CALIBRATION_TOL and c1["points"] == 4096
    m10, _ = _scaled_net(3, 10.0)
    st = m10.prepare(latent)
    c10 = m10.last_calibration
    assert c10["selected"] == "f32" and c10["max_abs_diff"] > 2.5e-5
    # the raw-logit rule rejected these weights: whatever the occupancy rule said (state kind), calls that return raw
    # logits run the exact kernels
    assert st.precision == "f32" or not st.logit_ok
    if st.precision == "f32":
        assert st.exact is None and c10["selected_occ"] == "f32"
    pts = torch.from_numpy(syn.seeded_cloud(53, 1, 700, -1.5, 1.5)).cuda()
    assert torch.equal(m10.query_points(st, pts), m10.query_points(m10.prepare(latent, "f32"), pts))
    axis9 = torch.linspace(-1.5, 1.5, 9).cuda()
    assert torch.equal(m10.query_grid(latent, axis9, apply_sigmoid=False, state=st),
                       m10.query_grid(latent, axis9, apply_sigmoid=False, state=m10.prepare(latent, "f32")))
    assert m10.prepare(latent, calibrate=False).precision == "f16x3"        # the unchecked state, for measurements
    m10.calibrate = False
    assert m10.prepare(latent).precision == "f16x3"
    # a NaN image first: fp32 state for that call, nothing cached, the next good image calibrates
    m2, _ = _scaled_net(2, 1.0)
    bad = latent.clone()
    bad[0, 3, 3] = float("nan")
    assert m2.prepare(bad).precision == "f32" and m2._calibration is None
    assert m2.prepare(latent).precision == "f16x3" and m2._calibration is not None


def _confident_net(seed, gain):
    """The seeded network with its last three MLP layers scaled so that every logit is ~gain x (synthetic.confident_state_dict)."""
    from zeroshape_amd.model.shape.implicit import Implicit
    from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed
    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(seed, pos_embed=pe).items()}
    sd = syn.confident_state_dict(sd, gain)
    m = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                 n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                 posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sd


@pytest.mark.parametrize("target", [10.0, 30.0, 100.0])
def test_logit_scale_sweep_on_the_seeded_network(target):
    """VERDICT r04 item 2 on the SEEDED network (the trained one: tests/test_gpu_trained_weights.py).  Scaling the last MLP
    layers multiplies every error by the gain, near the surface too - a harsher proxy than a trained checkpoint, whose large
    logits come from large activations far from the surface: here the raw-logit rule (2.5e-5) fails from |logit| ~ 5 and the
    occupancy rule (|d occ| <= 2.5e-5, no index flip outside the band) from ~ 35.  Whatever the verdicts: occupancy grids are
    within 1e-4 of the ORACLE with the oracle's occ > 0.5 index set outside the band, raw logits within 1e-4 relative; a call
    runs the split arithmetic exactly when the rule of the space it returns passed, otherwise the exact kernels, bit for bit;
    at |logit| ~ 10 the raw rule has failed and the occupancy grid still runs f16x3 with no tile sent to the fp32 kernel."""
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=1))
    gain, m, sd = 1.0, None, None
    for _ in range(4):                       # the scale is not exactly linear in the gain (unscaled biases upstream): iterate
        m, sd = _confident_net(0, gain)
        st = m.prepare(latent.cuda())
        cal = m.last_calibration
        assert cal is not None, "the scaled weights left the host envelope (W_MAX)"
        if 0.8 * target < cal["max_abs_logit"] < 1.25 * target:
            break
        gain *= target / cal["max_abs_logit"]
    assert 0.8 * target < cal["max_abs_logit"] < 1.25 * target
    occ_split = st.precision == "f16x3" and st.occ_ok
    assert occ_split == (cal["selected_occ"] == "f16x3") == (cal["max_abs_occ_diff"] <= m.CALIBRATION_TOL_OCC and cal["flips_outside_band"] == 0)
    if target == 10.0:
        assert occ_split and not st.logit_ok and st.image_flags_occ.cpu().tolist() == [0], cal
    N = 16
    grid = R.dense_grid(-1.5, 1.5, N)
    want_occ = R.level_grid(sd, latent, grid)                      # oracle occupancies [1, G, G, G]
    pts = grid.reshape(1, -1, 3)
    want_raw, _ = R.implicit_forward(sd, latent, pts)
    axis = torch.linspace(-1.5, 1.5, N + 1).cuda()
    st32 = m.prepare(latent.cuda(), "f32")
    occ = m.query_grid(latent.cuda(), axis, apply_sigmoid=True, state=st).cpu()
    if occ_split:
        assert m.last_tile_flags is not None and int(m.last_tile_flags.sum()) == 0     # no tile went to the exact kernel
    else:
        assert torch.equal(occ, m.query_grid(latent.cuda(), axis, apply_sigmoid=True, state=st32).cpu())
    assert float((occ - want_occ).abs().max()) < 1e-4
    outside = want_raw.reshape(occ.shape).abs() >= BAND * max(1.0, float(want_raw.abs().max()))
    assert torch.equal((occ > 0.5)[outside], (want_occ > 0.5)[outside])
    raw = m.query_grid(latent.cuda(), axis, apply_sigmoid=False, state=st).cpu()
    assert float((raw - want_raw.reshape(raw.shape)).abs().max()) < 1e-4 * max(1.0, float(want_raw.abs().max()))
    if st.precision == "f32" or not st.logit_ok:            # the raw rule failed: raw-logit calls are the exact kernels', bit for bit
        assert torch.equal(raw, m.query_grid(latent.cuda(), axis, apply_sigmoid=False, state=st32).cpu())
        assert torch.equal(m.query_points(st, pts.cuda()), m.query_points(st32, pts.cuda()))


def test_weights_beyond_w_max_select_the_exact_kernels():
    m, _ = _scaled_net(1, 1.0)
    with torch.no_grad():
        m.blocks_attn[0].mlp.fc2.weight[3, 5] = 40.0
    latent = torch.from_numpy(syn.seeded_latent(seed=1, batch=1)).cuda()
    st = m.prepare(latent)                 # asked for the default (f16x3), got the exact kernels
    assert st.precision == "f32" and st.exact is None
    with torch.no_grad():
        m.blocks_attn[0].mlp.fc2.weight[3, 5] = 0.04
    assert m.prepare(latent).precision == "f16x3"


def test_per_image_check_sends_an_outlier_image_to_the_exact_kernels():
    """the f16x3 verdict was measured on the first image seen and cached per weight version, while the
    error also depends on the image's K / V records.  prepare() now probes EVERY image through both kernels and flags, on the
    device, the ones beyond CALIBRATION_TOL: their tiles start flagged, so the fp32 launch behind every split launch
    re-evaluates them.  Here a network tuned close to the bound (attention weights x 5) calibrates on a normal image; in a
    batch of that image and the same latent scaled up until its probe error passes the bound, image 1 comes back as the exact
    kernel's numbers (within 1e-4 of the oracle), image 0 stays on the split arithmetic, bit for bit."""
    m, sd = None, None
    for gain in (4.0, 5.0, 6.0, 7.0):           # the largest gain whose own calibration still selects f16x3
        cand, csd = _scaled_net(3, gain)
        cand.precision = "f16x3"
        if cand.prepare(torch.from_numpy(syn.seeded_latent(seed=3, batch=1)).cuda()).precision != "f16x3":
            break
        m, sd = cand, csd
    assert m is not None
    base = torch.from_numpy(syn.seeded_latent(seed=3, batch=1)).cuda()
    pts = torch.from_numpy(syn.seeded_cloud(77, 2, 1500, -1.5, 1.5)).cuda()
    hit = None
    for scale in (1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0):
        lat = torch.cat([base, base * scale], 0)
        st = m.prepare(lat)
        assert st.precision == "f16x3" and st.image_flags is not None
        maxima = m.last_calibration["per_image_max_abs_diff"].cpu()
        assert maxima.shape == (2,) and float(maxima[0]) <= m.CALIBRATION_TOL
        if float(maxima[1]) > m.CALIBRATION_TOL:
            hit = (scale, lat, st)
            break
    assert hit is not None, "no latent scale pushed the split error past the bound"
    scale, lat, st = hit
    assert st.image_flags.cpu().tolist() == [0, 1]
    out = m.query_points(st, pts)
    exact = m.query_points(m.prepare(lat, "f32"), pts)
    alone = m.query_points(m.prepare(base, "f16x3", calibrate=False), pts[:1])
    assert torch.equal(out[1], exact[1]), "the flagged image must be the exact kernel's output"
    assert torch.equal(out[0], alone[0]), "the unflagged image stays on the split arithmetic"
    want, _ = R.implicit_forward(sd, lat[1:].cpu(), pts[1:].cpu())
    np.testing.assert_allclose(out[1:].cpu().numpy(), want.numpy(), atol=1e-4 * max(1.0, float(want.abs().max())), rtol=0)
    # the grid path honours the flags as well
    axis = torch.linspace(-1.5, 1.5, 9).cuda()
    g = m.query_grid(lat, axis, apply_sigmoid=False, state=st)
    ge = m.query_grid(lat, axis, apply_sigmoid=False, state=m.prepare(lat, "f32"))
    assert torch.equal(g[1], ge[1])
    # the multi-GPU step's prepare (parallel.prepare_sharded): image i is checked by rank i % W only.  Rank 1 of 2 finds the
    # outlier itself; rank 0 checks image 0 only and learns image 1's verdict from the exchange (here: a stand-in gather that
    # delivers what rank 1 measured); both then return what the unsharded state returned, bit for bit
    from zeroshape_amd import parallel

    def flags_of(state):          # (written on the check's side stream: this stream waits for its event, as the query paths do)
        torch.cuda.current_stream().wait_event(state.check_event)
        return state.image_flags.cpu().tolist()
    st1 = parallel.prepare_sharded(m, lat, rank=1, world_size=2, gather=parallel.solo_gather(1, 2))
    assert flags_of(st1) == [0, 1]
    mx = m.last_calibration["per_image_max_abs_diff"].cpu()
    assert float(mx[0]) == -1.0 and float(mx[1]) > m.CALIBRATION_TOL          # image 0 was not measured on this rank
    assert torch.equal(m.query_points(st1, pts), out)
    st0_alone = parallel.prepare_sharded(m, lat, rank=0, world_size=2, gather=parallel.solo_gather(0, 2))
    assert flags_of(st0_alone) == [0, 0]
    seen = []

    def gather_with_rank1(own):
        seen.append(own.cpu().clone())
        full = own.new_zeros((2,) + tuple(own.shape))
        full[0], full[1] = own, st1.image_flags.new_tensor([[1, 1]])
        return full
    st0 = parallel.prepare_sharded(m, lat, rank=0, world_size=2, gather=gather_with_rank1)
    assert flags_of(st0) == [0, 1] and seen[0].tolist() == [[0, 0]]
    assert torch.equal(m.query_points(st0, pts), out)
    assert torch.equal(m.query_grid(lat, axis, apply_sigmoid=False, state=st0), g)


def test_calibration_and_image_check_leave_the_callers_tile_flags_and_guard():
    """The calibration and the per-image check of prepare() measure the raw split arithmetic through the query path: that
    must neither replace the caller's last_tile_flags nor touch envelope_guard.  Batch 2 x 300 points: two full 128-point
    tiles and a 44-point tail per image."""
    m, _ = _scaled_net(3, 1.0)
    m.precision, m.calibrate, m.image_check = "f16x3", True, True
    latent = torch.from_numpy(syn.seeded_latent(seed=3, batch=2)).cuda()
    pts = torch.from_numpy(syn.seeded_cloud(91, 2, 300, -1.5, 1.5)).cuda()
    m.query_points(m.prepare(latent, calibrate=False), pts)          # guarded split query
    kept = m.last_tile_flags
    assert kept is not None and kept.shape == (2 * 3,)
    # other weights, their first call: _calibrate and _image_check both run
    m.load_state_dict(_scaled_net(5, 1.0)[1], strict=True)
    assert m._calibration is None
    st = m.prepare(latent)
    assert st.precision == "f16x3" and st.image_flags is not None and m._calibration is not None
    assert m.last_tile_flags is kept and m.envelope_guard is True


def test_verdict_statistics_of_both_output_spaces(net):
    """Implicit._verdict_stats (one launch of zs_sdf_verdict_stats per check): a confident network's raw error fails the raw
    rule while its occupancies agree; a flip counts only outside the band; a non-finite value fails both rules; the numbers
    equal the tensor-op formulation they replaced."""
    want = torch.tensor([[40.0, -35.0, 2e-6, -3e-4, 0.2]]).cuda()
    got = want + torch.tensor([[6e-5, -5e-5, -4e-6, 1e-6, 1e-6]]).cuda()      # index 2 flips inside the band
    st, fl = net._verdict_stats(got, want)
    assert abs(float(st[0, 0]) - 6e-5) < 4e-6 and float(st[0, 0]) > net.CALIBRATION_TOL          # raw rule fails (fp32 ulp at 40: 3.8e-6)
    assert float(st[0, 3]) <= net.CALIBRATION_TOL_OCC and float(st[0, 4]) == 0.0                 # occupancy rule passes
    assert fl.cpu().tolist() == [[1, 0]]
    got2 = want.clone()
    got2[0, 3] = 1e-6                                   # a flip at |logit| 3e-4: outside the band
    st2, fl2 = net._verdict_stats(got2, want)
    assert float(st2[0, 4]) == 1.0 and fl2.cpu().tolist() == [[1, 1]]           # (3.01e-4 of raw difference, and the flip)
    rs = np.random.RandomState(3)
    w = torch.from_numpy(rs.randn(3, 4096).astype(np.float32)).cuda()
    g = w + torch.from_numpy((1e-5 * rs.randn(3, 4096)).astype(np.float32)).cuda()
    g[1, 100] = float("nan")
    st3, fl3 = net._verdict_stats(g, w)
    d = (g - w).abs()
    ref = torch.stack([d.amax(-1), d.mean(-1), w.abs().amax(-1), (torch.sigmoid(g) - torch.sigmoid(w)).abs().amax(-1),
                       (((g > 0) != (w > 0)) & (w.abs() >= net.FLIP_BAND)).sum(-1).float()], -1)
    for b in (0, 2):
        np.testing.assert_allclose(st3[b].cpu().numpy(), ref[b].cpu().numpy(), rtol=1e-5, atol=1e-9)
    assert bool(torch.isnan(st3[1, :4]).all()) and fl3[1].cpu().tolist() == [1, 1]
    assert fl3[0].cpu().tolist() == [1 if float(ref[0, 0]) > net.CALIBRATION_TOL else 0,
                                     1 if float(ref[0, 3]) > net.CALIBRATION_TOL_OCC or float(ref[0, 4]) else 0]


def test_sharded_prepare_on_a_rank_without_an_image_of_its_own(net):
    """More ranks than images (evaluate.py --eval.shard_image with batch 1 on 8 GPUs): rank r > 0 checks nothing itself, still
    joins the exchange, and serves its point range with the verdict it received - the same numbers as the unsharded state."""
    from zeroshape_amd import parallel
    latent = torch.from_numpy(syn.seeded_latent(seed=4, batch=1)).cuda()
    axis = torch.linspace(-1.5, 1.5, 33).cuda()
    want = net.query_grid_range(latent, axis, 4096, 9000, state=net.prepare(latent))
    calls = []

    def gather(own):
        calls.append(own.cpu().clone())
        full = own.new_zeros((8,) + tuple(own.shape))
        full[3] = own                                  # this rank's (empty) contribution; rank 0's verdict: passed
        return full
    st = parallel.prepare_sharded(net, latent, rank=3, world_size=8, gather=gather)
    torch.cuda.current_stream().wait_event(st.check_event)
    assert len(calls) == 1 and calls[0].shape == (1, 2) and int(calls[0].abs().sum()) == 0
    assert st.image_flags.cpu().tolist() == [0] and st.precision == "f16x3"
    assert float(net.last_calibration["per_image_max_abs_diff"].cpu()[0]) == -1.0       # not measured on this rank
    assert torch.equal(net.query_grid_range(latent, axis, 4096, 9000, state=st), want)


def test_dynamic_tile_order_leaves_its_counter_at_zero_and_changes_no_value(net):
    """Round 4: the split kernels draw tiles from a counter in the workspace tail.  Launches of very different sizes back to
    back (fewer tiles than workgroups, one tile, many tiles, a grid) give the values a fresh workspace gives, and the counter is
    back at zero after each."""
    latent = torch.from_numpy(syn.seeded_latent(seed=5, batch=1)).cuda()
    dev = latent.device
    st = net.prepare(latent, "f16x3", calibrate=False)
    g = torch.Generator(device="cpu").manual_seed(3)
    outs = []
    for m in (5, 128, 129, 128 * 300 + 17, 1000):
        pts = (torch.rand(1, m, 3, generator=g) * 3 - 1.5).to(dev)
        outs.append((pts, net.query_points(st, pts)))
        torch.cuda.synchronize()
        from zeroshape_amd import _lib
        words = _lib.load().zs_sdf_workspace_bytes() // 4         # (the tensor may be longer: attention dumps live behind)
        counter = net.workspace(dev).view(torch.int32)[words - 1024 + 256]       # 1 KiB into the 4 KiB tail
        assert int(counter) == 0, (m, int(counter))
    net._workspace.clear()                                       # a fresh (zeroed) workspace
    for pts, want in outs:
        assert torch.equal(net.query_points(st, pts), want)


def test_tile_counter_is_the_librarys_and_the_static_deal_gives_the_same_values(net, monkeypatch):
    """the dynamic tile order trusted the caller to have zeroed the workspace.  Since ABI 33 the library resets
    its counter in front of every launch: a poisoned counter (garbage, negative) changes nothing, and ZS_SPLIT_STATIC_TILES=1
    (read per launch: tools/ab_tile_order.py alternates the arms in one process) evaluates the same tiles to the same bits."""
    from zeroshape_amd import _lib
    latent = torch.from_numpy(syn.seeded_latent(seed=6, batch=1)).cuda()
    st = net.prepare(latent, "f16x3", calibrate=False)
    pts = torch.from_numpy(syn.seeded_cloud(9, 1, 128 * 300 + 5, -1.5, 1.5)).cuda()
    want = net.query_points(st, pts)
    words = _lib.load().zs_sdf_workspace_bytes() // 4
    for poison in (123456789, -7, 2 ** 31 - 1):
        net.workspace(pts.device).view(torch.int32)[words - 1024 + 256] = poison
        assert torch.equal(net.query_points(st, pts), want), poison
    monkeypatch.setenv("ZS_SPLIT_STATIC_TILES", "1")
    assert torch.equal(net.query_points(st, pts), want)
    axis = torch.linspace(-1.5, 1.5, 33).cuda()
    g_static = net.query_grid(latent, axis, state=st)
    monkeypatch.delenv("ZS_SPLIT_STATIC_TILES")
    assert torch.equal(net.query_grid(latent, axis, state=st), g_static)
