"""The front end for several frames per call (frontend.frames_objects, the gp_frames_* entries) and
GenPose2.inference_frames on the device. Expected values: the numpy restatement (tests/frontend_ref.py) called once
per frame and concatenated (tests/frontend_frames_fixture.py), and frontend.frame_objects called per frame on the
device; the batch equals both bit for bit, no tolerances. roi_rgb, pts_center and zero_mean_pts, which the restatement
does not give in float32, are held to the per-frame device call bit for bit (test_gpu_frontend.py holds that call
to the restatement) and roi_rgb's uint8 levels to the restatement directly."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import frontend_frames_fixture as fx
import frontend_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = fx.H, fx.W
SIZES = [(56, 128), (112, 1024)]


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def batch(S, n_pts):
    """The three frames in one call: per-frame numpy inputs, a camera and a seed per frame."""
    from genpose2_amd.frontend import frames_objects
    out = frames_objects(*fx.frames(), list(fx.CAMERAS), img_size=S, n_pts=n_pts, max_depth=4.0, seed=list(fx.SEEDS),
                         device=DEV)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def per_frame(S, n_pts):
    """frame_objects on every frame by itself."""
    from genpose2_amd.frontend import frame_objects
    out = [frame_objects(*fx.frame(f), fx.CAMERAS[f], img_size=S, n_pts=n_pts, max_depth=4.0, seed=fx.SEEDS[f],
                         device=DEV) for f in range(3)]
    torch.cuda.synchronize()
    return out


def _same_rows(a, b, rows_a, rows_b, what):
    for k in fx.KEYS:
        if k != "frame":
            assert torch.equal(a[k][rows_a], b[k][rows_b]), (what, k)


def test_frames_mask_statistics_equal_numpy():
    from genpose2_amd import frontend
    masks = np.stack(fx.frames()[2])
    got = _np(frontend.frames_mask_stats(torch.from_numpy(masks).to(DEV)))
    assert got.shape == (3, 256, 5) and got.dtype == np.int32
    for f in range(3):
        assert np.array_equal(got[f], ref.mask_stats(masks[f])), f
        assert got[f, 1].tolist() == [0, H, -1, W, -1]           # an absent id
    assert got[1, 255].tolist() == [H * W, 0, H - 1, 0, W - 1] and not got[1, :255, 0].any()
    assert got[0, 7, 0] == 49 and got[2, 7, 0] == 25 * 30 and got[0, 7].tolist() != got[2, 7].tolist()
    # one frame through the same kernels, and frames wider than one row segment per thread, every id present
    assert np.array_equal(_np(frontend.mask_stats(torch.from_numpy(masks[2]).to(DEV))), got[2])
    rng = np.random.default_rng(1)
    masks = rng.integers(0, 256, (5, 67, 333), dtype=np.uint8)
    got = _np(frontend.frames_mask_stats(torch.from_numpy(masks).to(DEV)))
    assert all(np.array_equal(got[f], ref.mask_stats(masks[f])) for f in range(5))


@pytest.mark.parametrize("S,n_pts", SIZES)
def test_batch_equals_restatement_and_per_frame_calls(S, n_pts):
    want, got, single = fx.expected(S, n_pts), batch(S, n_pts), per_frame(S, n_pts)
    assert set(fx.KEYS) | {"frame_offsets", "pts_color", "pcl_in"} <= set(got)
    assert got["frame_offsets"] == want["frame_offsets"] == fx.OFFSETS
    assert got["frame"].dtype == torch.int32 and _np(got["frame"]).tolist() == want["frame"].tolist() == [0, 0, 0, 2, 2]
    assert got["ids"].dtype == torch.int32 and _np(got["ids"]).tolist() == want["ids"].tolist() == [0, 3, 7, 7, 9]
    assert got["count"].dtype == torch.int32 and np.array_equal(_np(got["count"]), want["count"])
    if S == 56:   # the 30 x 30 object selects, the 7 x 7 one tiles, in the same launch
        assert want["count"][1] > n_pts > want["count"][2]
    for k in ("roi_xs", "roi_ys"):
        assert got[k].dtype == torch.int32 and np.array_equal(_np(got[k]), want[k]), k
    pts = _np(got["pts"])
    assert pts.dtype == np.float32 and pts.shape == (5, n_pts, 3)
    assert np.array_equal(pts.view(np.uint32), want["pts"].view(np.uint32))
    assert got["pts_color"] is got["pts"] and got["pcl_in"] is got["pts"]
    assert (pts[..., 2] > 0).all() and (pts[..., 2] <= 4.0).all()
    # every key against frame_objects called per frame on the device
    for f in range(3):
        lo, hi = fx.OFFSETS[f], fx.OFFSETS[f + 1]
        assert single[f]["pts"].shape[0] == hi - lo
        _same_rows(got, single[f], slice(lo, hi), slice(None), f"frame {f}")
    assert got["roi_rgb"].shape == (5, 3, S, S) and got["roi_rgb"].dtype == torch.float32
    assert got["pts_center"].shape == (5, 3) and got["zero_mean_pts"].shape == (5, n_pts, 3)
    assert torch.equal(got["zero_mean_pts"], got["pts"] - got["pts_center"].unsqueeze(1))
    centre = _np(got["pts_center"]).astype(np.float64)
    assert np.abs(centre - want["pts_center"]).max() <= 1e-6 * np.abs(want["pts_center"]).max()
    # the colour crop's uint8 levels against the restatement on the object's own frame (values within 1e-3 of a
    # rounding boundary left out, as in test_gpu_frontend.py; the fixture's colour levels keep them rare)
    mean, std = np.array(ref.MEAN)[:, None, None], np.array(ref.STD)[:, None, None]
    rgb = _np(got["roi_rgb"]).astype(np.float64)
    skipped = total = 0
    for b, box in enumerate(want["boxes"]):
        norm, level, dist = ref.roi_rgb(fx.frame(int(want["frame"][b]))[1], box, S)
        keep = (dist > 1e-3).transpose(2, 0, 1)
        skipped, total = skipped + int((~keep).sum()), total + keep.size
        assert np.array_equal(np.rint((rgb[b] * std + mean) * 255.0)[keep], level.transpose(2, 0, 1)[keep]), b
        assert level.max() > 0
    assert skipped <= 0.01 * total


def test_frame_order_permutes_the_rows():
    """Frames 0 and 2 swapped (with their cameras and seeds): frame 2's rows first, no bit changed."""
    from genpose2_amd.frontend import frames_objects
    one = batch(56, 128)
    order = (2, 1, 0)
    swapped = frames_objects(*fx.frames(order=order), [fx.CAMERAS[f] for f in order], img_size=56, n_pts=128,
                             seed=[fx.SEEDS[f] for f in order], device=DEV)
    assert swapped["frame_offsets"] == [0, 2, 2, 5] and _np(swapped["frame"]).tolist() == [0, 0, 2, 2, 2]
    assert _np(swapped["ids"]).tolist() == [7, 9, 0, 3, 7]
    _same_rows(swapped, one, slice(0, 2), slice(3, 5), "frame 2 first")
    _same_rows(swapped, one, slice(2, 5), slice(0, 3), "frame 0 last")


def test_input_forms():
    from genpose2_amd.frontend import InferFrames, frame_objects, frames_objects
    one = batch(56, 128)
    depths, colors, masks = fx.frames()
    copies = [[a.copy() for a in x] for x in (depths, colors, masks)]
    # stacked tensors on the device (colour stays on the host), the reference's meta dictionaries
    stacked = frames_objects(torch.from_numpy(np.stack(copies[0])).to(DEV), torch.from_numpy(np.stack(copies[1])),
                             torch.from_numpy(np.stack(copies[2])).to(DEV),
                             [{"camera": {"intrinsics": c}} for c in fx.CAMERAS], img_size=56, n_pts=128,
                             seed=np.array(fx.SEEDS), device=DEV)
    # per-frame tensors on the device through InferFrames
    ds = InferFrames([{"depth": torch.from_numpy(d).to(DEV), "color": torch.from_numpy(c).to(DEV),
                       "mask": torch.from_numpy(m).to(DEV), "meta": k} for d, c, m, k in zip(*copies, fx.CAMERAS)],
                     img_size=56, device=DEV, n_pts=128)
    ds.seeds = list(fx.SEEDS)
    for other in (stacked, ds.get_objects()):
        assert other["frame_offsets"] == fx.OFFSETS and torch.equal(other["frame"], one["frame"])
        _same_rows(other, one, slice(None), slice(None), "input form")
    assert all(np.array_equal(a, b) for x, y in zip(copies, (depths, colors, masks)) for a, b in zip(x, y))
    # one shared camera and seed is that value repeated
    shared = frames_objects(depths, colors, masks, fx.CAM_B, img_size=56, n_pts=128, seed=23, device=DEV)
    repeated = frames_objects(depths, colors, masks, [fx.CAM_B] * 3, img_size=56, n_pts=128, seed=[23] * 3, device=DEV)
    _same_rows(shared, repeated, slice(None), slice(None), "shared camera and seed")
    assert not torch.equal(shared["pts"], one["pts"])
    # a 64-bit seed: the high half keys the sample too (frame 0, row 1 selects)
    hi = frames_objects(depths, colors, masks, list(fx.CAMERAS), img_size=56, n_pts=128,
                        seed=[fx.SEEDS[0] + (1 << 32), 5, 18], device=DEV)
    want = ref.frame_objects(*fx.frame(0), fx.CAM_A, 56, 128, 4.0, fx.SEEDS[0] + (1 << 32))
    assert np.array_equal(_np(hi["roi_xs"][:3]), want["roi_xs"]) and not torch.equal(hi["roi_xs"][1], one["roi_xs"][1])
    _same_rows(hi, one, slice(3, 5), slice(3, 5), "frame 2 beside another seed of frame 0")
    # F = 1 is frame_objects
    f1 = frames_objects(depths[2:], colors[2:], masks[2:], fx.CAM_B, img_size=56, n_pts=128, seed=18, device=DEV)
    single = frame_objects(depths[2], colors[2], masks[2], fx.CAM_B, img_size=56, n_pts=128, seed=18, device=DEV)
    assert f1["frame_offsets"] == [0, 2] and _np(f1["frame"]).tolist() == [0, 0]
    _same_rows(f1, single, slice(None), slice(None), "F = 1")


def test_frames_without_objects():
    from genpose2_amd.frontend import frame_objects, frames_objects
    empty = ((), (), ())
    out = frames_objects(*fx.frames(objects=empty), fx.CAM_A, img_size=56, n_pts=128, device=DEV)
    one = frame_objects(*fx.frame(1), fx.CAM_A, img_size=56, n_pts=128, device=DEV)
    assert out["frame_offsets"] == [0, 0, 0, 0]
    for k in fx.KEYS:
        if k != "frame":
            assert out[k].shape == one[k].shape and out[k].dtype == one[k].dtype and out[k].device == one[k].device, k
    assert out["frame"].shape == (0,) and out["frame"].dtype == torch.int32
    assert out["pts"].shape == (0, 128, 3) and out["roi_rgb"].shape == (0, 3, 56, 56)


def test_too_few_valid_points_names_frame_and_object():
    from genpose2_amd.frontend import frames_objects
    args = dict(img_size=56, n_pts=128, seed=list(fx.SEEDS), device=DEV)
    with_small = (fx.OBJECTS[0], (), fx.OBJECTS[2] + (fx.ID_SMALL,))
    with pytest.raises(ValueError, match=rf"frame 2, object id {fx.ID_SMALL} has \d valid points") as e:
        frames_objects(*fx.frames(objects=with_small), list(fx.CAMERAS), **args)
    assert "frame 0" not in str(e.value)
    both = (fx.OBJECTS[0] + (fx.ID_SMALL2,), (), fx.OBJECTS[2] + (fx.ID_SMALL,))
    with pytest.raises(ValueError) as e:
        frames_objects(*fx.frames(objects=both), list(fx.CAMERAS), **args)
    msg = str(e.value)
    assert f"frame 0, object id {fx.ID_SMALL2} has" in msg and f"frame 2, object id {fx.ID_SMALL} has" in msg
    # no valid pixel at all: frame 2's id 9 without depth
    depths, colors, masks = fx.frames()
    depths[2] = depths[2].copy()
    depths[2][masks[2] == 9] = 0
    with pytest.raises(ValueError, match="frame 2, object id 9 has 0 valid points"):
        frames_objects(depths, colors, masks, list(fx.CAMERAS), **args)


def test_frame_index_outside_the_call_reads_nothing():
    """The raw entries with frame_of = {0, 3, -1, 2, 1 << 30} for F = 3: the objects of frames 0 and 2 have their
    bits, the others count 0, zeroed points and indices, and colour level 0 (the crop of an image without pixels)."""
    from genpose2_amd import _lib, device as dev
    lib = _lib.load()
    one = batch(56, 128)
    S, n = 56, 128
    depths, colors, masks = (torch.from_numpy(np.stack(x)).to(DEV) for x in fx.frames())
    want = fx.expected(S, n)
    frame_of = torch.tensor([0, 3, -1, 2, 1 << 30], dtype=torch.int32, device=DEV)
    ids = one["ids"].clone()
    boxes = torch.tensor(np.array(want["boxes"], np.float32), device=DEV)
    intr = torch.tensor(np.array([ref.scaled_intrinsics(*(c[k] for k in ("fx", "fy", "cx", "cy", "width", "height")),
                                                        W, H) for c in fx.CAMERAS], np.float32), device=DEV)
    seeds = torch.tensor([[s, 0] for s in fx.SEEDS], dtype=torch.int32, device=DEV)
    pts = torch.full((5, n, 3), float("nan"), device=DEV)
    xs, ys = (torch.full((5, n), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    count = torch.full((5,), -7, dtype=torch.int32, device=DEV)
    rgb = torch.full((5, 3, S, S), float("nan"), device=DEV)
    ws_bytes = int(lib.gp_frame_objects_workspace_size(5, S))
    ws = torch.empty((ws_bytes // 4,), dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(dev.stream_handle(torch.device(DEV)))
    _lib.check(lib.gp_frames_objects(p(depths), p(masks), 3, H, W, p(frame_of), p(ids), p(boxes), 5, S, n, p(intr), 4.0,
                                     p(seeds), p(pts), p(xs), p(ys), p(count), p(ws), ws_bytes, st), "frames_objects")
    _lib.check(lib.gp_frames_roi_rgb(p(colors), 3, H, W, p(frame_of), p(boxes), 5, S, p(rgb), st), "frames_roi_rgb")
    torch.cuda.synchronize()
    for b in (0, 3):
        for k, t in (("pts", pts), ("roi_xs", xs), ("roi_ys", ys), ("count", count), ("roi_rgb", rgb)):
            assert torch.equal(t[b], one[k][b]), (b, k)
    level0 = torch.tensor([(0.0 - m) / s for m, s in zip(ref.MEAN, ref.STD)], dtype=torch.float64).float().to(DEV)
    for b in (1, 2, 4):
        assert int(count[b]) == 0 and not pts[b].any() and not xs[b].any() and not ys[b].any(), b
        assert torch.equal(rgb[b], level0[:, None, None].expand(3, S, S)), b


# ---------------------------------------------------------------------------- GenPose2.inference_frames
K_CAND = 20


def _cfg(**kw):
    from genpose2_amd.infer import default_config
    return default_config(device=DEV, sampling_steps=5, eval_repeat_num=K_CAND, noise_seed=3, **kw)


def _prev_pose(b):
    B = b["pts"].shape[0]
    g = torch.Generator().manual_seed(8)
    q = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)
    from genpose2_amd.aggregate import quaternion_to_matrix
    prev = torch.eye(4).repeat(B, 1, 1)
    prev[:, :3, :3] = quaternion_to_matrix(q)
    prev[:, :3, 3] = b["pts_center"].cpu() + 0.01 * torch.randn(B, 3, generator=g)
    return prev


def _split(t):
    return [t[lo:hi] for lo, hi in zip(fx.OFFSETS[:-1], fx.OFFSETS[1:])]


def test_inference_frames_splits_the_one_pipeline_call():
    from genpose2_amd.infer import GenPose2
    b = batch(56, 1024)
    torch.manual_seed(21)
    out = GenPose2(None, cfg=_cfg()).inference_frames(b)
    assert isinstance(out, list) and len(out) == 3
    for f, (pose, length) in enumerate(out):
        n = fx.OFFSETS[f + 1] - fx.OFFSETS[f]
        assert pose.shape == (n, 4, 4) and length.shape == (n, 3)
        assert torch.isfinite(pose).all() and torch.isfinite(length).all() and (length > 0).all()
        R = pose[:, :3, :3].double()
        if n:
            assert (R @ R.transpose(1, 2) - torch.eye(3, device=R.device, dtype=R.dtype)).abs().max() < 1e-5
        assert torch.equal(pose[:, 3], torch.tensor([0., 0., 0., 1.], device=pose.device).repeat(n, 1))
    assert out[1][0].shape == (0, 4, 4) and out[1][1].shape == (0, 3)
    # the same pipeline call as inference on the same batch dictionary
    torch.manual_seed(21)
    pose, length = GenPose2(None, cfg=_cfg()).inference(b)
    assert torch.equal(torch.cat([o[0] for o in out]), pose) and torch.equal(torch.cat([o[1] for o in out]), length)


def test_inference_frames_takes_infer_frames_and_warm_starts():
    from genpose2_amd.frontend import InferFrames
    from genpose2_amd.infer import GenPose2
    b = batch(56, 1024)
    prev = _prev_pose(b)
    ds = InferFrames([{"depth": d, "color": c, "mask": m, "meta": {"camera": {"intrinsics": k}}}
                      for d, c, m, k in zip(*fx.frames(), fx.CAMERAS)], img_size=56, device=DEV)
    ds.seeds = list(fx.SEEDS)
    torch.manual_seed(21)
    out = GenPose2(None, cfg=_cfg()).inference_frames(ds, prev_pose=_split(prev), tracking=True)
    torch.manual_seed(21)
    pose, length = GenPose2(None, cfg=_cfg()).inference(b, prev_pose=prev.to(DEV), tracking=True)
    assert [tuple(o[0].shape) for o in out] == [(3, 4, 4), (0, 4, 4), (2, 4, 4)]
    assert torch.equal(torch.cat([o[0] for o in out]), pose) and torch.equal(torch.cat([o[1] for o in out]), length)
    torch.manual_seed(21)
    cold, _ = GenPose2(None, cfg=_cfg()).inference(b)
    assert not torch.equal(cold, pose)                                  # the warm start is used
    gp = GenPose2(None, cfg=_cfg())
    with pytest.raises(ValueError, match="2 tensors for 3 frames"):
        gp.inference_frames(b, prev_pose=_split(prev)[:2])
    with pytest.raises(ValueError, match=r"prev_pose of frame 2 must be \(2,4,4\)"):
        gp.inference_frames(b, prev_pose=[prev[:3], prev[3:3], prev[3:4]])
    with pytest.raises(ValueError, match=r"prev_pose of frame 1 must be \(0,4,4\)"):
        gp.inference_frames(b, prev_pose=[prev[:3], prev[3:4], prev[3:5]])
    # every frame empty: F pairs of empty tensors, nothing run
    from genpose2_amd.frontend import frames_objects
    none = frames_objects(*fx.frames(objects=((), (), ())), fx.CAM_A, img_size=56, device=DEV)
    out = gp.inference_frames(none)
    assert [(tuple(p.shape), tuple(n.shape)) for p, n in out] == [((0, 4, 4), (0, 3))] * 3


def _frame2_rows(b):
    lo, hi = fx.OFFSETS[2], fx.OFFSETS[3]
    return {k: v[lo:hi].contiguous() for k, v in b.items() if isinstance(v, torch.Tensor)}


def _pred(agent, data, window):
    """pred_func with the agent's noise state restarted, as tests/test_gpu_ode_object.py does."""
    agent._calls = 0
    agent._gen.manual_seed(agent.cfg.noise_seed)
    agent.object_window = window
    try:
        pose, _ = agent.pred_func(data=dict(data), repeat_num=K_CAND, return_average_res=False, return_process=False)
    finally:
        agent.object_window = None
    torch.cuda.synchronize()
    return pose


def test_frames_do_not_couple_under_object_coupling():
    """ode_coupling='object': frame 2's candidates in the three-frame call are those of frame 2 alone (as a window
    of the same prior draw), bit for bit. Under the default batch coupling they are not."""
    from genpose2_amd.infer import GenPose2
    b = batch(56, 1024)
    lo, hi = fx.OFFSETS[2], fx.OFFSETS[3]
    agent = GenPose2(None, cfg=_cfg(ode_coupling="object")).score_agent
    whole = _pred(agent, b, None)
    alone = _pred(agent, _frame2_rows(b), (fx.OFFSETS[-1], lo))
    assert whole.shape[0] == 5 and alone.shape[0] == hi - lo and bool(torch.isfinite(whole).all())
    assert torch.equal(whole[lo:hi], alone)
    coupled = GenPose2(None, cfg=_cfg()).score_agent
    assert coupled.cfg.ode_coupling == "batch"
    assert not torch.equal(_pred(coupled, b, None)[lo:hi], _pred(coupled, _frame2_rows(b), None))
