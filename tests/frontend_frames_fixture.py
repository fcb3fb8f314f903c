"""The three 120 x 160 frames of the several-frames-per-call tests (test_cpu_frontend_frames.py,
test_gpu_frontend_frames.py), built by a seeded generator, and their expected batch: the numpy restatement
(tests/frontend_ref.py) called once per frame and concatenated.

  frame 0   ids 3 (30 x 30, interior), 7 (7 x 7) and 0 (bottom-right corner)   seed 17   camera A
  frame 1   background only                                                     seed 5    camera A
  frame 2   id 7 (25 x 30, elsewhere) and id 9 (30 x 40)                        seed 18   camera B

Every frame has its own depth holes and colours. ID_SMALL / ID_SMALL2 are 2 x 2 objects (fewer than 10 valid
points) that a test may add to a frame."""
import functools

import numpy as np

import frontend_ref as ref

H, W = 120, 160
CAM_A = dict(fx=411.3, fy=409.7, cx=158.6, cy=121.2, width=320, height=240)   # scaled by 0.5 to the frame
CAM_B = dict(fx=301.9, fy=305.2, cx=83.4, cy=57.7, width=160, height=120)     # the frame's own size
ID_SMALL, ID_SMALL2 = 200, 201
PLACES = (
    {3: (slice(40, 70), slice(50, 80)), 7: (slice(20, 27), slice(100, 107)), 0: (slice(100, 120), slice(135, 160)),
     ID_SMALL2: (slice(5, 7), slice(5, 7))},
    {},
    {7: (slice(60, 85), slice(20, 50)), 9: (slice(10, 40), slice(90, 130)), ID_SMALL: (slice(5, 7), slice(5, 7))},
)
OBJECTS = ((3, 7, 0), (), (7, 9))
SEEDS = (17, 5, 18)
CAMERAS = (CAM_A, CAM_A, CAM_B)
OFFSETS = [0, 3, 3, 5]
KEYS = ("pts", "roi_xs", "roi_ys", "count", "ids", "pts_center", "zero_mean_pts", "roi_rgb", "frame")


@functools.lru_cache(maxsize=None)
def frame(f, objects=None):
    """(depth, color, mask) of frame f with the given ids (default OBJECTS[f]): a tilted depth plane of the frame's
    own slope with 10 % holes and a patch beyond max_depth; colour levels that are multiples of 16, so that a
    bilinear value at the crops' 1/28-pixel positions never lies at a rounding boundary."""
    objects = OBJECTS[f] if objects is None else objects
    rng = np.random.default_rng(3000 + f)
    depth = (0.8 + 0.1 * f + (0.004 - 0.001 * f) * np.arange(W)[None, :]
             + (0.002 + 0.001 * f) * np.arange(H)[:, None]).astype(np.float32)
    depth[rng.random((H, W)) < 0.1] = 0
    depth[55:60, 65:70] = 5.0
    color = (16 * rng.integers(0, 16, (H, W, 3))).astype(np.uint8)
    mask = np.full((H, W), 255, np.uint8)
    for i in objects:
        mask[PLACES[f][i]] = i
    return depth, color, mask


def frames(objects=OBJECTS, order=(0, 1, 2)):
    """Per-frame lists (depths, colors, masks) of the frames in `order`."""
    return tuple(list(x) for x in zip(*(frame(f, tuple(objects[f])) for f in order)))


@functools.lru_cache(maxsize=None)
def expected_frame(f, S, n_pts):
    depth, color, mask = frame(f)
    return ref.frame_objects(depth, color, mask, CAMERAS[f], S, n_pts, 4.0, SEEDS[f])


@functools.lru_cache(maxsize=None)
def expected(S, n_pts):
    """The restatement frame by frame, concatenated: pts, roi_xs, roi_ys, count, ids, pts_center (float64), boxes,
    frame and frame_offsets."""
    per = [expected_frame(f, S, n_pts) for f in range(3)]
    out = {k: np.concatenate([p[k] for p in per]) for k in ("pts", "roi_xs", "roi_ys", "count", "ids", "pts_center")}
    # the restatement's empty frame holds float64 zeros of shape (0, ...): back to the dtypes of the others
    out["pts"] = out["pts"].astype(np.float32)
    out["roi_xs"], out["roi_ys"] = out["roi_xs"].astype(np.int32), out["roi_ys"].astype(np.int32)
    out["boxes"] =[b for p in per for b in p["boxes"]]
    out["frame"] = np.concatenate([np.full(len(p["ids"]), f, np.int32) for f, p in enumerate(per)])
    out["frame_offsets"] = np.concatenate([[0], np.cumsum([len(p["ids"]) for p in per])]).tolist()
    return out
