"""Block 0's point-side q/k/v from the rank-4 table on the GPU (csrc/sdf_decoder_split.hip: BLOCK 0 TABLE): the table
kernel against its host mirror, and the split decoder with block 0 from the compact stream built from that table (default)
and with block 0's q/k/v GEMMs (ZS_SPLIT_BLOCK0_GEMM=1, read per launch) against the exact-fp32 kernel and against each
other, at the bar of tests/test_gpu_decoder_split.py."""
import numpy as np
import pytest
import torch

from zeroshape_amd import program as P
from zeroshape_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ATOL = 1.5e-5   # tests/test_gpu_decoder_split.py: the split arithmetic against the exact-fp32 kernel (contract 1e-4)
BAND = 1e-5     # |logit| below which an occupancy flip is inside the arithmetic's error
ARMS = (("stream", None), ("gemm", "1"))


def _net(sd):
    from zeroshape_amd.model.shape.implicit import Implicit
    m = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                 n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                 posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def ctx(seeded_sd):
    """The seeded network, two images with different latents, their split and exact states (prepared once)."""
    net = _net(seeded_sd)
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2)).cuda()
    assert not torch.equal(latent[0], latent[1])
    return dict(net=net, latent=latent, split=net.prepare(latent, "f16x3", calibrate=False), exact=net.prepare(latent, "f32"))


def _arm(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("ZS_SPLIT_BLOCK0_GEMM", raising=False)
    else:
        monkeypatch.setenv("ZS_SPLIT_BLOCK0_GEMM", value)


def test_table_kernel_matches_the_mirror(ctx):
    """zs_sdf_block0_tables accumulates in double like the mirror (another summation order): rtol 1e-5 / atol 1e-6 are loose."""
    from zeroshape_amd import _lib
    st = ctx["split"]
    out = torch.full((2, P.B0_WINDOW_FLOATS), float("nan"), device="cuda")
    with _lib.on(out.device):
        rc = _lib.load().zs_sdf_block0_tables(_lib.ptr(st.programs), st.stride_bytes, 2, _lib.ptr(out),
                                              _lib.current_stream_ptr(out.device))
    _lib.check(rc, "zs_sdf_block0_tables")
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    for b in range(2):
        want = P.block0_window(st.programs[b].cpu().numpy().view(np.uint32))
        print("image %d: max |kernel - mirror| = %.3g" % (b, float(np.abs(got[b] - want).max())))
        np.testing.assert_allclose(got[b], want, rtol=1e-5, atol=1e-6)
        np.testing.assert_array_equal(got[b, :P.C], want[:P.C])           # b_proj: a copy
    assert np.array_equal(got[0], got[1])                                 # weights only: the latents do not enter


@pytest.mark.parametrize("m", [1, 33, 129])
def test_point_lists_both_arms_vs_fp32_kernel(ctx, monkeypatch, m):
    net = ctx["net"]
    pts = torch.from_numpy(syn.seeded_cloud(100 + m, 2, m, -1.5, 1.5)).cuda()
    exact = net.query_points(ctx["exact"], pts)
    got = {}
    for name, value in ARMS:
        _arm(monkeypatch, value)
        got[name] = net.query_points(ctx["split"], pts)
        assert got[name].shape == (2, m) and int(net.last_tile_flags.sum()) == 0
    err = {name: float((got[name] - exact).abs().max()) for name in got}
    d = float((got["stream"] - got["gemm"]).abs().max())
    print("m = %d: max |split - fp32| = %.3g (stream) %.3g (gemm), max |stream - gemm| = %.3g at max |logit| = %.3g" %
          (m, err["stream"], err["gemm"], d, float(exact.abs().max())))
    assert err["stream"] < ATOL and err["gemm"] < ATOL and d < ATOL
    if m == 129:
        assert not torch.equal(got["stream"], got["gemm"])                 # two arithmetics: the variable selects something
    assert not torch.equal(got["stream"][0], got["stream"][1])               # per-image latents are honoured


def test_grid33_and_point_range_both_arms(ctx, monkeypatch):
    """35,937 points = 281 tiles on at most 256 workgroups: some run a second tile through a re-initialised stream.  A point
    range that starts and ends inside a tile equals the grid's values bit for bit."""
    net, latent = ctx["net"], ctx["latent"][:1]
    G = 33
    axis = torch.linspace(-1.5, 1.5, G, device="cuda")
    from zeroshape_amd.model.shape.implicit import DecoderState
    exact_st = DecoderState(ctx["exact"].programs[:1], 1, "f32")
    split_st = DecoderState(ctx["split"].programs[:1], 1, "f16x3", exact=ctx["exact"].programs[:1])
    exact_occ = net.query_grid(latent, axis, apply_sigmoid=True, state=exact_st)
    exact_lg = net.query_grid(latent, axis, apply_sigmoid=False, state=exact_st)
    b, e = 1000 + 37, 9000 + 5
    assert b % 128 != 0
    occ = {}
    for name, value in ARMS:
        _arm(monkeypatch, value)
        occ[name] = net.query_grid(latent, axis, apply_sigmoid=True, state=split_st)
        assert occ[name].shape == (1, G, G, G) and int(net.last_tile_flags.sum()) == 0
        err = float((occ[name] - exact_occ).abs().max())
        flips = (occ[name] > 0.5) != (exact_occ > 0.5)
        print("grid 33, %s: max |split - fp32| = %.3g, %d occupancy disagreements" % (name, err, int(flips.sum())))
        assert err < ATOL
        assert bool(torch.all(exact_lg[flips].abs() < BAND))
        part = net.query_grid_range(latent, axis, b, e, apply_sigmoid=True, state=split_st)
        assert torch.equal(part, occ[name].reshape(1, -1)[:, b:e])
    d = float((occ["stream"] - occ["gemm"]).abs().max())
    print("grid 33: max |stream - gemm| = %.3g" % d)
    assert d < ATOL


def test_guard_fires_and_fp32_reevaluation_both_arms(monkeypatch):
    """(seed 3, gain 10, tol 1e-3) of test_other_weights_and_scales_vs_fp32_kernel with the envelope guard ON: q and k now come
    from the table (through the compact stream's rank-5 operands), the guard flags the tiles beyond the envelope and the exact
    kernel rewrites them.  Outputs are compared, not flag sets: a q that moved by 1e-7 may move a tile across the threshold."""
    from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed
    seed, gain, tol = 3, 10.0, 1e-3
    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(seed, pos_embed=pe).items()}
    for k in sd:
        if k.endswith("attn.qkv.weight") or k.endswith("mlp.fc1.weight") or k.endswith("latent_proj.weight"):
            sd[k] = sd[k] * gain
    m = _net(sd)
    assert m.envelope_guard
    latent = torch.from_numpy(syn.seeded_latent(seed=seed, batch=2)).cuda()
    pts = torch.from_numpy(syn.seeded_cloud(seed + 50, 2, 1500, -1.5, 1.5)).cuda()
    exact = m.query_points(m.prepare(latent, "f32"), pts)
    st = m.prepare(latent, "f16x3", calibrate=False)
    assert st.precision == "f16x3"
    scale = max(1.0, float(exact.abs().max()))
    for name, value in ARMS:
        _arm(monkeypatch, value)
        got = m.query_points(st, pts)
        flagged = int(m.last_tile_flags.sum())
        err = float((got - exact).abs().max())
        print("guard, %s: %d of %d tiles re-evaluated, max |final - fp32| = %.3g (scale %.3g)" %
              (name, flagged, m.last_tile_flags.numel(), err, scale))
        assert flagged > 0
        assert bool(torch.isfinite(got).all()) and err < tol * scale
