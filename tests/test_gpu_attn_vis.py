"""GPU: the attention heat-map frames of compute_level_grid(vis_attn=True) without the [G^3, 197] attention tensor -
z-mean attention of the drawn grid columns (zs_sdf_grid_attn_zmean, csrc/sdf_decoder.hip) against the oracle and against
the per-point map of the existing kernel, its chunking under a scratch cap, the frame composer (csrc/attn_vis.hip) against
its numpy restatement (tests/test_attn_vis_host_logic.py), the routing end to end, and the memory the path no longer takes.

Tolerance of a z-mean: 2e-7 (the per-row attention tolerance of test_gpu_decoder.py::test_attention_map_vs_oracle_ragged)
+ G * 2^-24 * max(want) (a sequential fp32 sum of G terms)."""
import numpy as np
import pytest
import torch

from oracle import decoder_ref as R
from tests.test_attn_vis_host_logic import compose_ref
from zeroshape_amd import synthetic as syn

pytestmark = pytest.mark.gpu

CASES = {17: 2, 33: 1}        # G -> batch: several columns per 128-point tile at heavy padding / one point past a wave tile


def _implicit(seeded_sd, precision=None):
    from zeroshape_amd.model.shape.implicit import Implicit
    m = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                 n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                 posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    m.load_state_dict(seeded_sd, strict=True)
    m = m.cuda().eval()
    if precision is not None:
        m.precision = precision
    return m


@pytest.fixture(scope="module")
def net(seeded_sd):
    return _implicit(seeded_sd, "f32")       # the exact-fp32 kernels, as in test_gpu_decoder.py


@pytest.fixture(scope="module")
def net_default(seeded_sd):
    return _implicit(seeded_sd)              # the default arithmetic (f16x3 with its fp32 programs kept for the map)


def _tol(G, want):
    return 2e-7 + G * 2.0 ** -24 * float(want.max())


def _case(G):
    """latent [B,197,C], axis [G], columns [n,2], the columns' points [B, n * G, 3] (all CPU)."""
    from zeroshape_amd.utils.eval_3D import attention_frame_columns
    B = CASES[G]
    latent = torch.from_numpy(syn.seeded_latent(seed=5, batch=2))[:B]
    axis = torch.linspace(-1.5, 1.5, G)
    columns, _ = attention_frame_columns(G)
    ix = torch.from_numpy(columns[:, 0].astype(np.int64))
    iy = torch.from_numpy(columns[:, 1].astype(np.int64))
    n = len(columns)
    pts = torch.stack([axis[ix][:, None].expand(n, G), axis[iy][:, None].expand(n, G), axis[None].expand(n, G)], -1)
    return latent, axis, columns, pts.reshape(1, n * G, 3).repeat(B, 1, 1).contiguous()


_ORACLE = {}


def _oracle_zmean(seeded_sd, G):
    """The oracle's attention of the columns' points, averaged over z: [B, n_cols, 197].  Computed once per G."""
    if G not in _ORACLE:
        latent, _, columns, pts = _case(G)
        _, attn = R.implicit_forward(seeded_sd, latent, pts)
        _ORACLE[G] = attn.view(latent.shape[0], len(columns), G, 197).mean(2).numpy()
    return _ORACLE[G]


@pytest.mark.parametrize("G", sorted(CASES))
def test_zmean_vs_oracle(net, seeded_sd, G):
    latent, axis, columns, _ = _case(G)
    want = _oracle_zmean(seeded_sd, G)
    got = net.query_grid_attention(latent.cuda(), axis.cuda(), columns)
    assert got.shape == want.shape and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy() - want).max())
    print("G=%d  max |zmean - oracle| = %.3e  (bound %.3e, max %.3e)" % (G, err, _tol(G, want), want.max()))
    assert err <= _tol(G, want)
    if CASES[G] > 1:
        assert float(np.abs(want[0] - want[1]).max()) > 100 * _tol(G, want)       # the images really differ


@pytest.mark.parametrize("G", sorted(CASES))
def test_zmean_vs_per_point_attention_of_the_device(net, G):
    latent, axis, columns, pts = _case(G)
    _, attn = net(latent.cuda(), None, pts.cuda(), need_attn=True)
    want = attn.view(latent.shape[0], len(columns), G, 197).mean(2).cpu().numpy()
    got = net.query_grid_attention(latent.cuda(), axis.cuda(), columns).cpu().numpy()
    err = float(np.abs(got - want).max())
    print("G=%d  max |zmean - mean of device rows| = %.3e  (bound %.3e)" % (G, err, _tol(G, want)))
    assert err <= _tol(G, want)


@pytest.mark.parametrize("G", sorted(CASES))
def test_chunked_equals_single_chunk_bit_for_bit(net, G):
    from zeroshape_amd import _lib
    lib = _lib.load()
    latent, axis, columns, _ = _case(G)
    B, n = latent.shape[0], len(columns)
    latent, axis = latent.cuda(), axis.cuda()
    state = net.prepare(latent)
    assert net.grid_attention_chunks(B, n, G)[2] == 1                               # the default cap: one chunk
    one = net.query_grid_attention(latent, axis, columns, state=state)
    assert torch.equal(one, net.query_grid_attention(latent, axis, columns, state=state))     # run to run
    uncapped = lib.zs_sdf_grid_attn_zmean_scratch_bytes(B, n, G, 1 << 62)
    cap = uncapped // 4
    imgs, cols, chunks = net.grid_attention_chunks(B, n, G, cap)
    assert chunks >= 3 and chunks == -(-B // imgs) * -(-n // cols)
    assert 0 < lib.zs_sdf_grid_attn_zmean_scratch_bytes(B, n, G, cap) <= cap
    got = net.query_grid_attention(latent, axis, columns, state=state, scratch_cap_bytes=cap)
    assert torch.equal(got, one)
    with pytest.raises(_lib.ZeroShapeHipError):           # below one wave tile's raw dump (495,616 bytes)
        net.query_grid_attention(latent, axis, columns, state=state, scratch_cap_bytes=400000)


def _band(scaled):
    """Pixels whose heat-map level may legitimately differ: 255 v / m within 1e-3 of an integer (10x the few-ulp error
    of an operation-for-operation restatement at values up to 255)."""
    return np.abs(scaled - np.round(scaled)) <= 1e-3


@pytest.mark.parametrize("size", [(224, 224, 16), (48, 80, 3)])       # 14 x 14 patches; H != W with 16 x 16 patches
def test_composer_vs_numpy_restatement(size):
    from zeroshape_amd.utils import eval_3D as E
    from zeroshape_amd.utils.options import EasyDict as edict
    H, W, win = size
    Rr = H // win
    opt = edict(dict(device="cuda", H=H, W=W, arch=dict(win_size=win)))
    rs = np.random.RandomState(H)
    zmean = rs.uniform(0.003, 0.008, (2, 3, 1 + Rr * Rr)).astype(np.float32)
    images = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H))
    frame_col = np.array([2, 0, 1, 2], np.int32)
    got = E.attention_frames(opt, torch.from_numpy(zmean).cuda(), frame_col, images.cuda())
    assert got.shape == (2, 4, H, W, 3) and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got, E.attention_frames(opt, torch.from_numpy(zmean).cuda(), frame_col, images.cuda()))
    got = got.cpu().numpy()
    lut = E._jet_lut()
    worst = 0.0
    for b in range(2):
        for f, c in enumerate(frame_col):
            want, scaled = compose_ref(zmean[b, c], images[b].numpy(), lut, Rr, H, W)
            band = _band(scaled)
            assert band.mean() <= 0.01, "the seeded input puts %.2f %% of a frame inside the band" % (100 * band.mean())
            # outside the band the levels agree (a level apart is >= 1/255/2 in some channel) and so do the pixels
            err = float(np.abs(got[b, f] - want)[~band].max())
            worst = max(worst, err)
            assert err <= 1e-6, (b, f, err)
            assert abs(float(got[b, f].max()) - 1.0) <= 1e-6 and got[b, f].min() >= 0
    print("%dx%d  max |frame - restatement| outside the band = %.3e" % (H, W, worst))
    with pytest.raises(AssertionError):
        E.attention_frames(opt, torch.from_numpy(zmean).cuda(), frame_col, 2 * images.cuda())


def test_level_grid_frames_end_to_end(net_default, seeded_sd):
    """vox 16 on the default arithmetic: the occupancies are those of every other call, the frames those of the oracle's
    attention, and the slice loop (an untagged copy of the grid) draws the same frames."""
    from zeroshape_amd.utils import eval_3D as E
    from zeroshape_amd.utils.options import EasyDict as edict
    G = 17
    latent = torch.from_numpy(syn.seeded_latent(seed=5, batch=2))[:CASES[G]].cuda()
    B = latent.shape[0]
    opt = edict(dict(device="cuda", H=224, W=224, eval=dict(vox_res=G - 1, range=[-1.5, 1.5]), arch=dict(win_size=16)))
    grid = E.get_dense_3D_grid(opt, edict(dict(idx=list(range(B)))))
    images = torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    occ, frames = E.compute_level_grid(opt, net_default, latent, None, grid, images, vis_attn=True)
    occ_plain, none = E.compute_level_grid(opt, net_default, latent, None, grid, None, vis_attn=False)
    assert none is None and torch.equal(occ, occ_plain)
    columns, frame_col = E.attention_frame_columns(G)
    assert len(frames) == B and all(len(fr) == len(frame_col) == 9 for fr in frames)
    assert all(f.shape == (224, 224, 3) and f.dtype == np.float32 for fr in frames for f in fr)
    zmean = _oracle_zmean(seeded_sd, G)
    lut = E._jet_lut()
    for b in range(B):
        for f, c in enumerate(frame_col):
            want, _ = compose_ref(zmean[b, c], images[b].cpu().numpy(), lut, 14, 224, 224)
            assert float(np.abs(frames[b][f] - want).max()) < 2e-2        # (one level of the heat map can move)
    _, loop = E.compute_level_grid(opt, net_default, latent, None, grid.clone(), images, vis_attn=True)
    assert len(loop) == B and all(len(fr) == 9 for fr in loop)
    for b in range(B):
        for f in range(9):
            assert float(np.abs(loop[b][f] - frames[b][f]).max()) < 2e-2


def test_level_grid_frames_do_not_hold_the_attention_tensor(net):
    """vox 96, 169 columns: the peak above what was allocated before the call stays below the one [97^3, 197] fp32 tensor
    the slice loop stacks (and holds twice): by accounting the capped scratch (256 MiB) + the frames (102 MB)."""
    from zeroshape_amd.utils import eval_3D as E
    from zeroshape_amd.utils.options import EasyDict as edict
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=1)).cuda()
    opt = edict(dict(device="cuda", H=224, W=224, eval=dict(vox_res=96, range=[-1.5, 1.5]), arch=dict(win_size=16)))
    grid = E.get_dense_3D_grid(opt, edict(dict(idx=[0])))
    images = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    occ, frames = E.compute_level_grid(opt, net, latent, None, grid, images, vis_attn=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("vox 96: peak above the call's start = %.1f MB (bound %.1f MB)" % (peak / 1e6, 97 ** 3 * 197 * 4 / 1e6))
    assert occ.shape == (1, 97, 97, 97) and len(frames[0]) == 169
    assert peak < 97 ** 3 * 197 * 4


def test_argument_handling(net, seeded_sd):
    from zeroshape_amd.model.shape.implicit import Implicit
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2)).cuda()
    axis = torch.linspace(-1.5, 1.5, 17).cuda()
    out = net.query_grid_attention(latent, axis, np.zeros((0, 2), np.int32))
    assert out.shape == (2, 0, 197) and out.dtype == torch.float32
    with pytest.raises(IndexError):
        net.query_grid_attention(latent, axis, np.array([[0, 17]], np.int32))
    sem = Implicit(syn.NUM_PATCHES, latent_dim=2 * syn.LATENT_DIM, semantic=True, n_channels=syn.N_CHANNELS,
                   n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                   posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False).cuda().eval()
    with pytest.raises((ValueError, NotImplementedError)):
        sem.query_grid_attention(torch.cat([latent, latent], -1), axis, np.array([[0, 0]], np.int32))
