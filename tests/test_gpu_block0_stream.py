"""Block 0 from its compact stream on the GPU (csrc/sdf_decoder_split.hip: BLOCK 0 STREAM): the stream kernel against its
host mirror, and the split decoder's two block-0 arms - compact stream (default) and GEMMs (ZS_SPLIT_BLOCK0_GEMM=1, read per
launch, and every launch of more than 175 images) - against the exact-fp32 kernel and against each other, at the bars of
tests/test_gpu_block0_tables.py."""
import numpy as np
import pytest
import torch

from zeroshape_amd import program as P
from zeroshape_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ATOL = 1.5e-5   # tests/test_gpu_block0_tables.py, tests/test_gpu_decoder_split.py: split arithmetic vs the exact-fp32 kernel
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
    """The seeded network, two images with different latents, their split and exact states, and the exact kernel's 33^3
    grid of the first image (prepared once, never modified)."""
    from zeroshape_amd.model.shape.implicit import DecoderState
    net = _net(seeded_sd)
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2)).cuda()
    assert not torch.equal(latent[0], latent[1])
    split, exact = net.prepare(latent, "f16x3", calibrate=False), net.prepare(latent, "f32")
    axis = torch.linspace(-1.5, 1.5, 33, device="cuda")
    exact1 = DecoderState(exact.programs[:1], 1, "f32")
    split1 = DecoderState(split.programs[:1], 1, "f16x3", exact=exact.programs[:1])
    return dict(net=net, latent=latent, split=split, exact=exact, axis=axis, split1=split1,
                exact_occ=net.query_grid(latent[:1], axis, apply_sigmoid=True, state=exact1),
                exact_lg=net.query_grid(latent[:1], axis, apply_sigmoid=False, state=exact1))


def test_stream_kernel_matches_the_mirror(ctx):
    """zs_sdf_block0_streams against program.block0_stream on the device's own table.  Copied K-blocks and the q, k, v operands
    (the table's values, split) are bit-equal.  The U operands are sums in double in the mirror's order, but fused on the
    device, so a float rounding may fall the other way: hi + lo / s is compared at the rtol / atol of
    test_table_kernel_matches_the_mirror, and the share of bit-equal words is printed."""
    from zeroshape_amd import _lib
    st = ctx["split"]
    tables = torch.full((2, P.B0_WINDOW_FLOATS), float("nan"), device="cuda")
    streams = torch.full((2, P.B0S_WORDS), -1, dtype=torch.int32, device="cuda")
    with _lib.on(tables.device):
        lib, sp = _lib.load(), _lib.current_stream_ptr(tables.device)
        _lib.check(lib.zs_sdf_block0_tables(_lib.ptr(st.programs), st.stride_bytes, 2, _lib.ptr(tables), sp), "zs_sdf_block0_tables")
        _lib.check(lib.zs_sdf_block0_streams(_lib.ptr(st.programs), st.stride_bytes, 2, _lib.ptr(tables), _lib.ptr(streams), sp),
                   "zs_sdf_block0_streams")
    got = streams.cpu().numpy().view(np.uint32).reshape(2, P.B0S_KB, P.KB_WORDS)
    slots = P.block0_stream_slots()

    def value(half_words):
        """[64 lanes][8] fp16 of a packed operand -> the rows' hi + lo / s, [32][5] float64"""
        h = np.ascontiguousarray(half_words).view(np.float16).reshape(64, 8).astype(np.float64)
        hi = np.concatenate([h[:32, :4], h[32:, 4:5]], axis=1)
        lo = np.concatenate([h[32:, :4], h[32:, 6:7]], axis=1)
        return hi + lo / P.B0S_LO_SCALE
    for b in range(2):
        words = st.programs[b].cpu().numpy().view(np.uint32)
        want = P.block0_stream(words, window=tables[b].cpu().numpy()).reshape(P.B0S_KB, P.KB_WORDS)
        same = total = 0
        for h in range(P.HEADS):
            for i, s in enumerate(slots):
                g, w = got[b, h * P.B0S_KB_HEAD + i], want[h * P.B0S_KB_HEAD + i]
                if s[0] == "copy":
                    np.testing.assert_array_equal(g, w)
                    continue
                for half, op in enumerate(s[1:]):
                    gh, wh = g[half * 256:(half + 1) * 256], w[half * 256:(half + 1) * 256]
                    if op < 3:
                        np.testing.assert_array_equal(gh, wh)
                    else:
                        np.testing.assert_allclose(value(gh), value(wh), rtol=1e-5, atol=1e-6)
                        same, total = same + int((gh == wh).sum()), total + gh.size
        print("image %d: %d of %d words of the U operands bit-equal to the mirror" % (b, same, total))
    assert not np.array_equal(got[0], got[1])                                # K and V are the image's


@pytest.mark.parametrize("m", [1, 33, 128, 129, 300])
def test_point_lists_both_arms_vs_fp32_kernel(ctx, monkeypatch, m):
    net = ctx["net"]
    pts = torch.from_numpy(syn.seeded_cloud(200 + m, 2, m, -1.5, 1.5)).cuda()
    exact = net.query_points(ctx["exact"], pts)
    got = {}
    for name, env in ARMS:
        _arm(monkeypatch, env)
        got[name] = net.query_points(ctx["split"], pts)
        assert got[name].shape == (2, m) and int(net.last_tile_flags.sum()) == 0
    err = {name: float((got[name] - exact).abs().max()) for name in got}
    d = float((got["stream"] - got["gemm"]).abs().max())
    print("m = %d: max |split - fp32| = %s, between arms %.3g, max |logit| = %.3g" % (m, err, d, float(exact.abs().max())))
    assert all(e < ATOL for e in err.values()) and d < ATOL
    if m >= 128:
        assert not torch.equal(got["stream"], got["gemm"])                  # another arithmetic: the variable selects something
    assert not torch.equal(got["stream"][0], got["stream"][1])                # per-image latents are honoured


def test_grid33_and_point_range_both_arms(ctx, monkeypatch):
    """35,937 points = 281 tiles on at most 256 workgroups: some workgroups re-enter the compact stream for a second tile.  A
    point range that starts and ends inside a tile equals the grid's values bit for bit."""
    net, latent, axis, st = ctx["net"], ctx["latent"][:1], ctx["axis"], ctx["split1"]
    b, e = 1000 + 37, 9000 + 5
    occ = {}
    for name, env in ARMS:
        _arm(monkeypatch, env)
        occ[name] = net.query_grid(latent, axis, apply_sigmoid=True, state=st)
        assert occ[name].shape == (1, 33, 33, 33) and int(net.last_tile_flags.sum()) == 0
        err = float((occ[name] - ctx["exact_occ"]).abs().max())
        flips = (occ[name] > 0.5) != (ctx["exact_occ"] > 0.5)
        print("grid 33, %s: max |split - fp32| = %.3g, %d occupancy disagreements" % (name, err, int(flips.sum())))
        assert err < ATOL
        assert bool(torch.all(ctx["exact_lg"][flips].abs() < BAND))
        part = net.query_grid_range(latent, axis, b, e, apply_sigmoid=True, state=st)
        assert torch.equal(part, occ[name].reshape(1, -1)[:, b:e])
    d = float((occ["stream"] - occ["gemm"]).abs().max())
    print("grid 33: max |stream - gemm| = %.3g" % d)
    assert d < ATOL


def test_identical_launches_are_bit_equal(ctx, monkeypatch):
    _arm(monkeypatch, {})
    net, latent, axis, st = ctx["net"], ctx["latent"][:1], ctx["axis"], ctx["split1"]
    a = net.query_grid(latent, axis, apply_sigmoid=False, state=st).clone()
    b = net.query_grid(latent, axis, apply_sigmoid=False, state=st)
    assert torch.equal(a, b)


def test_u_beyond_fp16_flags_the_tile_for_the_fp32_kernel(seeded_sd, monkeypatch):
    """point_proj scaled by 1e-6: the point rows' variance vanishes against LayerNorm's eps = 1e-6, so rstd = 1,000 for every
    point and rstd x = 1e5 > 65,504 at x = 100.  The compact-stream arm flags that point's tile (and no other: |rstd x| <=
    1,500 elsewhere), and the exact kernel's re-evaluation returns its own values there."""
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


@pytest.fixture(scope="module")
def many(seeded_sd):
    """176 images - one more than block0_stream_fit allows - prepared once: the split state, and its fp32 programs as an
    exact state (2 x 176 x 10.16 MB)."""
    from zeroshape_amd.model.shape.implicit import DecoderState
    n = 176
    assert P.block0_stream_fit(n - 1) and not P.block0_stream_fit(n)
    net = _net(seeded_sd)
    latent = torch.from_numpy(syn.seeded_latent(seed=5, batch=n)).cuda()
    split = net.prepare(latent, "f16x3", calibrate=False)
    assert split.precision == "f16x3"
    return dict(net=net, n=n, split=split, exact=DecoderState(split.exact, n, "f32"))


def _images(state, idx):
    """The split state of the images `idx` (a list) of `state`, or of its first `idx` images (an int)."""
    from zeroshape_amd.model.shape.implicit import DecoderState
    if isinstance(idx, int):
        return DecoderState(state.programs[:idx], idx, "f16x3", exact=state.exact[:idx])
    return DecoderState(state.programs[idx].contiguous(), len(idx), "f16x3", exact=state.exact[idx].contiguous())


@pytest.mark.parametrize("m", [1, 129])
def test_more_images_than_streams_fit_take_the_gemm_arm(many, monkeypatch, m):
    """176 images in one launch: the tables and streams no longer fit the workspace's head, and block 0 runs its q/k/v GEMMs.
    A point's value does not depend on the batch it rode in (same tile position, same wave, same lane), so images 0 and 175 of
    that launch are bit-equal to a 2-image launch of their programs under ZS_SPLIT_BLOCK0_GEMM=1 - and, at 129 points, not to
    the 2-image launch of the stream arm.  175 images still take the stream: images 0 and 174 are bit-equal to the stream
    arm's 2-image launch (and, at 129 points, not to the GEMM arm's)."""
    net, n, st = many["net"], many["n"], many["split"]
    pts = torch.from_numpy(syn.seeded_cloud(400 + m, n, m, -1.5, 1.5)).cuda()
    _arm(monkeypatch, {})
    got = net.query_points(st, pts)
    assert got.shape == (n, m) and int(net.last_tile_flags.sum()) == 0
    err = float((got - net.query_points(many["exact"], pts)).abs().max())
    print("m = %d, %d images: max |split - fp32| = %.3g" % (m, n, err))
    assert err < ATOL
    got175 = net.query_points(_images(st, n - 1), pts[:n - 1])
    assert int(net.last_tile_flags.sum()) == 0
    pair = {}
    for ends in ([0, n - 1], [0, n - 2]):
        for name, env in ARMS:
            _arm(monkeypatch, env)
            pair[name, ends[1]] = net.query_points(_images(st, ends), pts[ends].contiguous())
    assert torch.equal(got[[0, n - 1]], pair["gemm", n - 1])
    assert torch.equal(got175[[0, n - 2]], pair["stream", n - 2])
    if m == 129:
        assert not torch.equal(got[[0, n - 1]], pair["stream", n - 1])
        assert not torch.equal(got175[[0, n - 2]], pair["gemm", n - 2])
