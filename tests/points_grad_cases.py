"""The configurations, seeded inputs and error measures shared by tests/golden/make_points_grad_golden.py (the reference's
`Implicit` differentiated in its query points) and the tests that read its file (tests/test_points_grad_host_logic.py,
tests/test_gpu_points_grad.py).  No test in here."""
import numpy as np

from zeroshape_amd import synthetic as syn

B, M = 2, 333
FACTOR = 8.0            # a gradient may differ from the fp64 one by FACTOR x what the reference's own fp32 gradient does
SKIP_BELOW = 1e-3       # angle checks leave out vertices whose |g64| is below SKIP_BELOW x the median ...
SKIP_MOST = 0.01        # ... and no more than this fraction of them

CASES = {
    # options/shape.yaml
    "yaml": dict(ctor=dict(num_patches=syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                           n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS, posenc_3D=0,
                           mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False),
                 syn=dict(), seed=0, sem=0, inputs=2),
    # ... with the NeRF encoding in front of the per-point MLP (27 channels, padded to 28)
    "posenc4": dict(ctor=dict(num_patches=syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                              n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS, posenc_3D=4,
                              mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False),
                    syn=dict(posenc_3D=4), seed=0, sem=0, inputs=1),
    # a prediction head instead of the MLP, semantic codes, 3 blocks ("head" of make_variants_golden.py)
    "head": dict(ctor=dict(num_patches=49, latent_dim=128, semantic=True, n_channels=128, n_blocks_attn=3, n_layers_mlp=0,
                           num_heads=4, mlp_ratio=2.0, pos_perlayer=False),
                 syn=dict(n_channels=128, latent_dim=128, att_blocks=3, mlp_ratio=2.0, mlp_layers=0, skip_in=(), num_patches=49),
                 seed=3, sem=32, inputs=0),
}
# Not in the golden file: the GPU tests' edge shapes also run 9 point channels (padded to 12) against the oracle.
EXTRA = {
    "posenc1": dict(ctor=dict(CASES["yaml"]["ctor"], posenc_3D=1), syn=dict(posenc_3D=1), seed=0, sem=0, inputs=3),
}


def case(name):
    return CASES[name] if name in CASES else EXTRA[name]


def inputs(name, batch=B, m=M):
    """(latent_depth [batch,L,C - sem], latent_semantic [batch,L,sem] | None, points [batch,m,3] in [-0.6, 0.6]^3, cotangent
    [batch,m]) as float32 arrays: the latents and clouds of zeroshape_amd/synthetic.py."""
    cfg = case(name)
    k, n_sem = cfg["inputs"], cfg["sem"]                   # (k: the seed of this case's latents, cloud and cotangent)
    tokens = cfg["ctor"]["num_patches"] + 1
    dim = cfg["ctor"]["latent_dim"]
    lat = syn.seeded_latent(seed=k, batch=batch, n_tokens=tokens, dim=dim)
    sem = None
    if n_sem:
        lat, sem = np.ascontiguousarray(lat[..., :dim - n_sem]), np.ascontiguousarray(lat[..., dim - n_sem:])
    pts = syn.seeded_cloud(seed=k, batch=batch, n=m, lo=-0.6, hi=0.6)
    cot = np.random.RandomState(31 + k).randn(batch, m).astype(np.float32)
    return lat, sem, pts, cot


def state_dict(name, pos_embed):
    return syn.seeded_state_dict(seed=case(name)["seed"], pos_embed=pos_embed, **case(name)["syn"])


def rel_error(g, g64):
    """max |g - g64| / max |g64|."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return float(np.abs(g - g64).max() / np.abs(g64).max())


def normal_angles(g, g64):
    """(largest angle in degrees between -g/|g| and -g64/|g64| over the rows that count, fraction of rows left out): rows whose
    |g64| is below SKIP_BELOW x the median |g64| are left out."""
    g, g64 = np.asarray(g, np.float64).reshape(-1, 3), np.asarray(g64, np.float64).reshape(-1, 3)
    n64 = np.linalg.norm(g64, axis=1)
    keep = n64 >= SKIP_BELOW * np.median(n64)
    a, b = g[keep] / np.linalg.norm(g[keep], axis=1, keepdims=True), g64[keep] / n64[keep, None]
    # (atan2 of |a x b| and a . b: acos loses half the digits at these angles)
    ang = np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1)))
    return float(ang.max()) if keep.any() else 0.0, float(1.0 - keep.mean())
