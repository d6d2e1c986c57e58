"""LN2's output in registers (csrc/sdf_decoder_split.hip: LN2 IN REGISTERS): fc1 of both attention blocks takes its B operands
from the accumulator half of the register file instead of the wave's LDS slab.  The values and their order are unchanged, so
the split decoder is held to the bars of tests/test_gpu_block0_stream.py at the same shapes, under both block-0 arms (compact
stream, and ZS_SPLIT_BLOCK0_GEMM=1 where `head` and LN1 run in block 0 as well), and its two fences - a component of u beyond
the fp16 range, a tile beyond the S_GUARD envelope - still hand their tiles to the exact-fp32 kernel."""
import pytest
import torch

from zeroshape_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ATOL = 1.5e-5   # tests/test_gpu_block0_stream.py: split arithmetic vs the exact-fp32 kernel
BAND = 1e-5     # |logit| below which an occupancy flip is inside the arithmetic's error
ARMS = (("stream", {}), ("gemm", {"ZS_SPLIT_BLOCK0_GEMM": "1"}))


def _net(sd):
    from zeroshape_amd.model.shape.implicit import Implicit
    m = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                 n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                 posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _arm(monkeypatch, env):
    monkeypatch.delenv("ZS_SPLIT_BLOCK0_GEMM", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def ctx(seeded_sd):
    """The seeded network, two images with different latents, their split (calibrated) and exact states, and the exact
    kernel's 33^3 grid of the first image (prepared once, never modified)."""
    from zeroshape_amd.model.shape.implicit import DecoderState
    net = _net(seeded_sd)
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2)).cuda()
    assert not torch.equal(latent[0], latent[1])
    split, exact = net.prepare(latent), net.prepare(latent, "f32")
    axis = torch.linspace(-1.5, 1.5, 33, device="cuda")
    exact1 = DecoderState(exact.programs[:1], 1, "f32")
    split1 = DecoderState(split.programs[:1], 1, "f16x3", exact=exact.programs[:1])
    return dict(net=net, latent=latent, split=split, exact=exact, axis=axis, split1=split1,
                exact_occ=net.query_grid(latent[:1], axis, apply_sigmoid=True, state=exact1),
                exact_lg=net.query_grid(latent[:1], axis, apply_sigmoid=False, state=exact1))


def test_calibration_still_selects_f16x3(ctx):
    assert ctx["split"].precision == "f16x3"


@pytest.mark.parametrize("arm", ARMS, ids=[a[0] for a in ARMS])
@pytest.mark.parametrize("images", [1, 2])
@pytest.mark.parametrize("m", [1, 33, 128, 129, 300])
def test_point_lists_vs_fp32_kernel(ctx, monkeypatch, m, images, arm):
    """Ragged last tiles (1, 33, 129, 300), a whole tile (128), and tile counts (1 to 6) far below the grid."""
    from zeroshape_amd.model.shape.implicit import DecoderState
    net = ctx["net"]
    pts = torch.from_numpy(syn.seeded_cloud(200 + m, 2, m, -1.5, 1.5)).cuda()[:images].contiguous()
    split = DecoderState(ctx["split"].programs[:images], images, "f16x3", exact=ctx["exact"].programs[:images])
    exact = net.query_points(DecoderState(ctx["exact"].programs[:images], images, "f32"), pts)
    _arm(monkeypatch, arm[1])
    got = net.query_points(split, pts)
    assert got.shape == (images, m) and int(net.last_tile_flags.sum()) == 0
    err = float((got - exact).abs().max())
    print("m = %d, %d image(s), %s: max |split - fp32| = %.3g at max |logit| = %.3g" %
          (m, images, arm[0], err, float(exact.abs().max())))
    assert err < ATOL
    if images == 2:
        assert not torch.equal(got[0], got[1])                                # per-image latents are honoured


@pytest.mark.parametrize("arm", ARMS, ids=[a[0] for a in ARMS])
def test_grid33_vs_fp32_kernel_and_bit_reproducible(ctx, monkeypatch, arm):
    """35,937 points = 281 tiles on at most 256 workgroups: a tile count the grid does not divide.  Two identical launches are
    bit-equal."""
    net, latent, axis, st = ctx["net"], ctx["latent"][:1], ctx["axis"], ctx["split1"]
    _arm(monkeypatch, arm[1])
    occ = net.query_grid(latent, axis, apply_sigmoid=True, state=st)
    assert occ.shape == (1, 33, 33, 33) and int(net.last_tile_flags.sum()) == 0
    err = float((occ - ctx["exact_occ"]).abs().max())
    flips = (occ > 0.5) != (ctx["exact_occ"] > 0.5)
    print("grid 33, %s: max |split - fp32| = %.3g, %d occupancy disagreements" % (arm[0], err, int(flips.sum())))
    assert err < ATOL
    assert bool(torch.all(ctx["exact_lg"][flips].abs() < BAND))
    a = net.query_grid(latent, axis, apply_sigmoid=False, state=st).clone()
    b = net.query_grid(latent, axis, apply_sigmoid=False, state=st)
    assert torch.equal(a, b)
    err = float((a - ctx["exact_lg"]).abs().max())
    print("grid 33, %s, raw logits: max |split - fp32| = %.3g" % (arm[0], err))
    assert err < ATOL


def test_u_beyond_fp16_still_flags_the_tile_for_the_fp32_kernel(seeded_sd, monkeypatch):
    """The set-up of tests/test_gpu_block0_stream.py: point_proj scaled by 1e-6, so rstd = 1,000 for every point and
    rstd x = 1e5 > 65,504 at x = 100.  The compact-stream arm flags that point's tile and no other, and the exact kernel's
    re-evaluation returns its own values there."""
    sd = {k: v.clone() for k, v in seeded_sd.items()}
    sd["point_proj.proj.weight"] *= 1e-6
    sd["point_proj.proj.bias"] *= 1e-6
    net = _net(sd)
    assert net.envelope_guard
    latent = torch.from_numpy(syn.seeded_latent(seed=2, batch=2)).cuda()
    pts = torch.from_numpy(syn.seeded_cloud(77, 2, 300, -1.5, 1.5)).cuda()
    pts[0, 200, 0] = 100.0                                                    # image 0, tile 1 (points 128..255)
    exact = net.query_points(net.prepare(latent, "f32"), pts)
    st = net.prepare(latent, "f16x3", calibrate=False)
    assert st.precision == "f16x3"
    _arm(monkeypatch, {})
    got = net.query_points(st, pts)
    flags = net.last_tile_flags.reshape(2, 3).cpu()
    other = torch.ones(2, 300, dtype=torch.bool)
    other[0, 128:256] = False
    print("u beyond fp16: flags %s, max |split - fp32| on the other tiles %.3g" %
          (flags.tolist(), float((got - exact).abs().cpu()[other].max())))
    assert flags.tolist() == [[0, 1, 0], [0, 0, 0]]
    assert bool(torch.isfinite(got).all()) and torch.equal(got[0, 128:256], exact[0, 128:256])
    assert float((got - exact).abs().cpu()[other].max()) < ATOL


@pytest.mark.parametrize("arm", ARMS, ids=[a[0] for a in ARMS])
def test_s_guard_still_sends_flagged_tiles_to_the_fp32_kernel(seeded_sd, monkeypatch, arm):
    """q/k, fc1 and latent_proj weights x10 (the set-up of tests/test_gpu_decoder_split.py's guard test, on the seeded
    network): some point's d^-1/2 |q| max |k| exceeds S_GUARD, its tile is flagged, and the guarded result is the exact
    kernel's there and the raw split kernel's everywhere else, bit for bit."""
    sd = {k: v.clone() for k, v in seeded_sd.items()}
    for k in sd:
        if k.endswith("attn.qkv.weight") or k.endswith("mlp.fc1.weight") or k.endswith("latent_proj.weight"):
            sd[k] = sd[k] * 10.0
    net = _net(sd)
    assert net.envelope_guard
    latent = torch.from_numpy(syn.seeded_latent(seed=3, batch=2)).cuda()
    pts = torch.from_numpy(syn.seeded_cloud(53, 2, 1500, -1.5, 1.5)).cuda()
    st = net.prepare(latent, "f16x3", calibrate=False)
    exact = net.query_points(net.prepare(latent, "f32"), pts)
    _arm(monkeypatch, arm[1])
    guarded = net.query_points(st, pts)
    flags = net.last_tile_flags.clone().view(2, -1).bool()
    print("S_GUARD, %s: %d of %d tiles flagged" % (arm[0], int(flags.sum()), flags.numel()))
    assert flags.shape[1] == 12 and bool(flags.any())
    net.envelope_guard = False
    raw = net.query_points(st, pts)
    per_point = flags.repeat_interleave(128, dim=1)[:, :1500]
    assert torch.equal(guarded[per_point], exact[per_point])
    assert torch.equal(guarded[~per_point], raw[~per_point])
