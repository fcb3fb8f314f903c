"""Cases, seeds, weights and inputs of the image encoder's edge tests (test_cpu_img_edge.py, test_gpu_img_edge.py): the
--dino pointwise image branch (gp_imgenc.hip, and the implicit-im2col form of linear_split_kernel) off its one shape
(B, 256, 384): grids smaller than a wave and than a GEMM tile, partial 64 x 64 tiles, ragged softmax tails, a batch of
one object more than an edge chunk, a near one-hot geometric softmax, an all-zero object. Nothing is stored: weights and
inputs come from seeds, and the float64 / float32 references are computed by tests/img_ref.py when a test asks."""
from __future__ import annotations

import functools
import warnings

import numpy as np

IE_EDGE_CHUNK = 256      # objects per im2col GEMM of the column-buffer path (gp_imgenc.hip)
GEMM_TILE = 64           # bgemm_nt_kernel's output tile (rows and columns)
WAVE = 64                # lanes: a softmax row is read 64 keys at a time
WEIGHT_SEED = 4100
PREFIX = "img_encoder"
# the embedding's centre row (the table entry of i == j, which multiplies |G_i|^2 > 0) sums to this: the diagonal
# logit grows with the square of the input scale, which is what makes "sharp" sharp
CENTRE_SUM = 2.0
OUTPUTS = ("final", "layer_w", "edge")

# name -> (B, grid, d, input scale); np = grid^2. The input seed is INPUT_SEED0 + the case's position.
CASES = {
    "g4":          (3, 4, 64, 0.3),      # np = 16 < a wave and < a GEMM tile; K = np = 16: one k-group; co = 16; d < 256
    "g8":          (2, 8, 128, 0.2),     # np = 64: exactly one wave and one tile, no tails
    "g12":         (3, 12, 64, 0.3),     # np = 144 = 2 * 64 + 16: partial tile rows / columns, softmax tail of 16
    "g12_wide":    (1, 12, 384, 0.12),   # the production width on an off grid, B = 1
    "g20":         (2, 20, 64, 0.3),     # np = 400 > 256: seven tile rows; 1444 embedding rows < 39^2: the clamp is live
    "chunk":       (257, 4, 64, 0.3),    # one object past IE_EDGE_CHUNK
    "chunk2":      (513, 4, 64, 0.3),    # two full chunks and one object
    "sharp":       (2, 12, 64, 1.0),     # g12's weights, a larger input: near one-hot geometric softmax
    "zero_obj":    (3, 4, 64, 0.3),      # object 1 is all zeros in all three layers
    "same_layers": (2, 8, 128, 0.2),     # l0 = l1 = l2
}
INPUT_SEED0 = 4200
# what each case is there for: np, its remainder in GEMM tiles and in 64-lane softmax steps, whole tiles per side,
# K of the values GEMM in 16-deep k-groups, conv outputs co, objects in the last edge chunk and the number of chunks,
# d % 256 (pixel max / gather step), the number of (i, j) table entries whose index lies past the default embedding's
# last row (the clamp acts on them)
PROPERTIES = {
    "g4":          dict(np=16, tile_rem=16, tiles=1, wave_rem=16, kgroups=1, co=16, chunks=1, last_chunk=3, d_mod256=64, clamped=46),
    "g8":          dict(np=64, tile_rem=0, tiles=1, wave_rem=0, kgroups=4, co=32, chunks=1, last_chunk=2, d_mod256=128, clamped=190),
    "g12":         dict(np=144, tile_rem=16, tiles=3, wave_rem=16, kgroups=9, co=16, chunks=1, last_chunk=3, d_mod256=64, clamped=430),
    "g12_wide":    dict(np=144, tile_rem=16, tiles=3, wave_rem=16, kgroups=9, co=96, chunks=1, last_chunk=1, d_mod256=128, clamped=430),
    "g20":         dict(np=400, tile_rem=16, tiles=7, wave_rem=16, kgroups=25, co=16, chunks=1, last_chunk=2, d_mod256=64, clamped=1198),
    "chunk":       dict(np=16, tile_rem=16, tiles=1, wave_rem=16, kgroups=1, co=16, chunks=2, last_chunk=1, d_mod256=64, clamped=46),
    "chunk2":      dict(np=16, tile_rem=16, tiles=1, wave_rem=16, kgroups=1, co=16, chunks=3, last_chunk=1, d_mod256=64, clamped=46),
    "sharp":       dict(np=144, tile_rem=16, tiles=3, wave_rem=16, kgroups=9, co=16, chunks=1, last_chunk=2, d_mod256=64, clamped=430),
    "zero_obj":    dict(np=16, tile_rem=16, tiles=1, wave_rem=16, kgroups=1, co=16, chunks=1, last_chunk=3, d_mod256=64, clamped=46),
    "same_layers": dict(np=64, tile_rem=0, tiles=1, wave_rem=0, kgroups=4, co=32, chunks=1, last_chunk=2, d_mod256=128, clamped=190),
}
# objects compared on their own at the chunk boundaries
CHUNK_PROBES = {"chunk": (255, 256), "chunk2": (255, 256, 511, 512)}


def _raw_table_index(g: int) -> np.ndarray:
    """(c_j - c_i + g - 1) . (2 g - 1, 1) before any clamp: (np, np)."""
    p = np.arange(g * g)
    return ((p[None, :] // g - p[:, None] // g + g - 1) * (2 * g - 1)
            + p[None, :] % g - p[:, None] % g + g - 1)


def case_properties(name: str) -> dict:
    """PROPERTIES[name] recomputed from the case's shape and the kernels' constants."""
    b, g, d, _ = CASES[name]
    n = g * g
    return dict(np=n, tile_rem=n % GEMM_TILE, tiles=-(-n // GEMM_TILE), wave_rem=n % WAVE, kgroups=n // 16, co=d // 4,
                chunks=-(-b // IE_EDGE_CHUNK), last_chunk=b - (b - 1) // IE_EDGE_CHUNK * IE_EDGE_CHUNK, d_mod256=d % 256,
                clamped=int((_raw_table_index(g) > (2 * (g - 1)) ** 2 - 1).sum()))


def _state_dict(d: int, grid: int, seed: int, emb_rows=None) -> dict:
    if d % 64 or grid < 2:
        raise ValueError("d must be a multiple of 64 and grid >= 2")
    rng = np.random.Generator(np.random.PCG64([seed, d, grid]))
    hid, co = d // 2, d // 4
    rows = (2 * (grid - 1)) ** 2 if emb_rows is None else int(emb_rows)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    n = rng.standard_normal
    sd = {
        "layer_attn.0.weight": f(n((hid, d)) * np.sqrt(2.0 / d)),
        "layer_attn.0.bias": f(n(hid) * 0.1),
        "layer_attn.2.weight": f(n((1, hid)) * (4.0 / np.sqrt(hid))),
        "layer_attn.2.bias": f(n(1) * 0.1),
        "rel_pos_emb.weight": f(n((rows, co)) / np.sqrt(co)),          # row sums ~ N(0, 1)
        "edge_guide.0.weight": f(n((co, d, 3, 3)) * np.sqrt(2.0 / (9 * d))),
        "edge_guide.0.bias": f(n(co) * 0.1),
        "geo_weight": np.array(0.5 + 0.5 * rng.random(), np.float32),
        "edge_weight": np.array(0.5 + 0.5 * rng.random(), np.float32),
    }
    centre = 2 * grid * (grid - 1)         # the index of c_j == c_i: (g - 1) (2 g - 1) + g - 1
    if centre < rows:
        e = sd["rel_pos_emb.weight"]
        e[centre] += np.float32((CENTRE_SUM - float(e[centre].astype(np.float64).sum())) / co)
    out = {f"{PREFIX}.{k}": v for k, v in sd.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def state_dict(d: int, grid: int, seed: int = WEIGHT_SEED, emb_rows=None) -> dict:
    """An ``img_encoder.*`` state dict with the reference's key names at width d on a grid x grid map: layer_attn.0
    (d/2, d), layer_attn.2 (1, d/2), rel_pos_emb (emb_rows, d/4) -- by default the reference's undersized
    (2 (grid - 1))^2 rows, so geo_table's clamp acts --, edge_guide.0 (d/4, d, 3, 3), positive geo_weight and
    edge_weight. Weights are scaled by fan-in; the embedding's centre row sums to CENTRE_SUM."""
    return _state_dict(d, grid, seed, emb_rows)


def case_state_dict(name: str) -> dict:
    _, g, d, _ = CASES[name]
    return state_dict(d, g, WEIGHT_SEED)


def raw_layers(name: str):
    """The case's three layers before zero_obj / same_layers edit them."""
    b, g, d, scale = CASES[name]
    rng = np.random.Generator(np.random.PCG64(INPUT_SEED0 + list(CASES).index(name)))
    x = rng.standard_normal((3, b, g * g, d)).astype(np.float32) * np.float32(scale)
    return [x[0], x[1], x[2]]


@functools.lru_cache(maxsize=None)
def _layers(name: str):
    ls = raw_layers(name)
    if name == "zero_obj":
        for v in ls:
            v[1] = 0.0
    if name == "same_layers":
        ls = [ls[0], ls[0], ls[0]]
    for v in ls:
        v.setflags(write=False)
    return tuple(ls)


def layers(name: str):
    """Three (B, grid^2, d) float32 arrays (read-only, shared) from one PCG64 stream per case, times its scale."""
    return list(_layers(name))


def rel(a, b) -> float:
    """max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def yardstick(sd: dict, ls, grid: int) -> dict:
    """The float64 restatement's outputs and eps[output] = the error of oracle.img_encoder_forward (fp32, CPU) against
    them, relative to max |ref| of that output: {"ref": {final, layer_w, edge, fused}, "eps": {final, layer_w, edge}}."""
    import img_ref
    from oracle import oracle
    ref = img_ref.img_encoder_forward64(sd, ls, grid)
    with warnings.catch_warnings():     # torch.from_numpy of the shared read-only arrays (nothing writes to them)
        warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
        final, parts = oracle.img_encoder_forward(sd, ls, return_parts=True)
    got = {"final": final, "layer_w": parts["layer_w"].transpose(0, 2, 1), "edge": parts["edge"]}
    eps = {k: rel(got[k], ref[k]) for k in OUTPUTS}
    for v in ref.values():
        v.setflags(write=False)
    return {"ref": ref, "eps": eps}


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """yardstick() of a case, computed once per process and shared by every form and test."""
    return yardstick(case_state_dict(name), layers(name), CASES[name][1])


# ---------------------------------------------------------------- gp_gather_patch_points
# (B, np, grid, patch, d, N): d in {4, 64, 260, 384, 1024}, N in {1, 3, 4, 5, 1023}, the three square grids and one
# mismatched pair (np = 100 on a grid of 16: the clamp to np - 1 acts on in-image points), patch in {1, 14, 16}
GATHER_CASES = (
    (2, 16, 4, 1, 4, 1),
    (3, 16, 4, 16, 64, 3),
    (1, 256, 16, 14, 260, 4),
    (2, 256, 16, 14, 384, 1023),
    (2, 400, 20, 16, 1024, 5),
    (3, 400, 20, 1, 64, 1023),
    (2, 100, 16, 14, 64, 5),
    (1, 100, 16, 16, 260, 1023),
)
GATHER_SEED0 = 4300


def gather_specials(grid: int, patch: int):
    """(x, y) pairs every case with room for them starts with: exactly -1, -patch and -patch - 1 on either axis, and
    xs in range with ys = -1 (the combined index is clamped, not each axis: that is the previous row's last patch)."""
    p, g = patch, grid
    return ((0, -1), (-1, 0), (2 * p, -1), ((g - 1) * p, -1), (-p, p), (p, -p), (-p - 1, 2 * p), (3 * p, -p - 1),
            (-1, -1), ((g + 3) * p - 1, (g + 3) * p - 1), (-3 * p, -3 * p), ((g - 1) * p, g * p), (g * p, 0))


def gather_inputs(i: int):
    """feat (B, np, d) float32, xs, ys (B, N) int32 in [-3 patch, (grid + 3) patch) of GATHER_CASES[i]."""
    b, n_p, grid, patch, d, n = GATHER_CASES[i]
    rng = np.random.Generator(np.random.PCG64(GATHER_SEED0 + i))
    feat = rng.standard_normal((b, n_p, d)).astype(np.float32)
    xs = rng.integers(-3 * patch, (grid + 3) * patch, size=(b, n)).astype(np.int32)
    ys = rng.integers(-3 * patch, (grid + 3) * patch, size=(b, n)).astype(np.int32)
    sp = gather_specials(grid, patch)
    # rotate the list by the case's position so that the small cases (B N < the list) start at different pairs
    sp = (sp[i % len(sp):] + sp[:i % len(sp)])[:b * n]
    fx, fy = xs.reshape(-1), ys.reshape(-1)
    for j, (x, y) in enumerate(sp):
        fx[j], fy[j] = x, y
    return feat, xs, ys
