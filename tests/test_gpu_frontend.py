"""The RGB-D front end and GenPose2.inference on the device against the numpy restatement
(tests/frontend_ref.py) on one seeded synthetic frame."""
import functools

import numpy as np
import pytest
import torch

import frontend_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 120, 160
ID_A, ID_B, ID_C, ID_D, ID_E = 3, 7, 0, 200, 9
INTR = dict(fx=411.3, fy=409.7, cx=158.6, cy=121.2, width=320, height=240)   # scaled by 0.5 to the frame
SEED = 17


@functools.lru_cache(maxsize=None)
def frame(objects=(ID_A, ID_B, ID_C)):
    """depth: a tilted plane with holes and a patch beyond max_depth; the colour levels are multiples of 16, so
    that a bilinear value at the crops' 1/28-pixel positions is a multiple of 1/49 and never lies at a rounding
    boundary; objects A (30 x 30, interior), B (7 x 7), C (in the bottom-right corner), D (2 x 2); E (80 x 80, over A's place: used alone) fills the
    largest window, so that its crop at S = 280 holds more than 2^16 valid pixels."""
    rng = np.random.default_rng(2024)
    depth = (0.8 + 0.004 * np.arange(W)[None, :] + 0.002 * np.arange(H)[:, None]).astype(np.float32)
    depth[rng.random((H, W)) < 0.1] = 0
    depth[55:60, 65:70] = 5.0
    color = (16 * rng.integers(0, 16, (H, W, 3))).astype(np.uint8)
    mask = np.full((H, W), 255, np.uint8)
    where = {ID_A: (slice(40, 70), slice(50, 80)), ID_B: (slice(20, 27), slice(100, 107)),
             ID_C: (slice(100, 120), slice(135, 160)), ID_D: (slice(5, 7), slice(5, 7)),
             ID_E: (slice(20, 100), slice(30, 110))}
    for i in objects:
        mask[where[i]] = i
    return depth, color, mask


@functools.lru_cache(maxsize=None)
def expected(objects, S, n_pts, seed=SEED):
    depth, color, mask = frame(objects)
    return ref.frame_objects(depth, color, mask, INTR, S, n_pts, 4.0, seed)


@functools.lru_cache(maxsize=None)
def device_batch(objects, S, n_pts, seed=SEED):
    from genpose2_amd.frontend import frame_objects
    depth, color, mask = frame(objects)
    out = frame_objects(depth, color, mask, INTR, img_size=S, n_pts=n_pts, max_depth=4.0, seed=seed, device=DEV)
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.cpu().numpy()


def test_mask_statistics_equal_numpy():
    from genpose2_amd import frontend
    for objects in ((ID_A, ID_B, ID_C), (ID_A, ID_B, ID_C, ID_D), ()):
        mask = frame(objects)[2]
        got = _np(frontend.mask_stats(torch.from_numpy(mask.copy()).to(DEV)))
        want = ref.mask_stats(mask)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert want[1].tolist() == [0, H, -1, W, -1]           # an absent id
    # a frame wider than one row segment per thread and no multiple of it, every id present
    rng = np.random.default_rng(1)
    mask = rng.integers(0, 256, (67, 333), dtype=np.uint8)
    assert np.array_equal(_np(frontend.mask_stats(torch.from_numpy(mask).to(DEV))), ref.mask_stats(mask))
    # more row segments than the grid has threads (256 x 256): every thread walks several
    mask = np.array([255, 0, 4, 254], np.uint8)[rng.integers(0, 4, (1100, 1003))]
    mask[:3] = 255
    mask[:700][mask[:700] == 254] = 255
    assert np.array_equal(_np(frontend.mask_stats(torch.from_numpy(mask).to(DEV))), ref.mask_stats(mask))


# the last case: the largest n_pts, and element positions beyond 2^16 (a third byte of e in the selection)
CASES = [((ID_A, ID_B, ID_C), 56, 128), ((ID_A, ID_B, ID_C), 112, 128), ((ID_A,), 224, 1024), ((ID_E,), 280, 2048)]


@pytest.mark.parametrize("objects,S,n_pts", CASES)
def test_frame_objects_equal_restatement(objects, S, n_pts):
    want = expected(objects, S, n_pts)
    got = device_batch(objects, S, n_pts)
    assert _np(got["ids"]).tolist() == sorted(objects) == want["ids"].tolist()
    assert np.array_equal(_np(got["count"]), want["count"])
    if ID_A in objects:
        assert want["count"][sorted(objects).index(ID_A)] > n_pts    # A takes the selection path
    else:
        assert want["count"][0] > 1 << 16
    if ID_B in objects and S == 56:
        assert want["count"][sorted(objects).index(ID_B)] < n_pts    # B the tiling path
    if S == 112:   # C's window lies on the border: nearest source indices reach H and W
        assert want["outside"][sorted(objects).index(ID_C)]
    for k in ("roi_xs", "roi_ys"):
        assert got[k].dtype == torch.int32 and np.array_equal(_np(got[k]), want[k]), k
    pts = _np(got["pts"])
    assert pts.dtype == np.float32 and pts.shape == (len(objects), n_pts, 3)
    assert np.array_equal(pts.view(np.uint32), want["pts"].astype(np.float32).view(np.uint32))
    assert got["pts_color"] is got["pts"] and got["pcl_in"] is got["pts"]
    centre = _np(got["pts_center"]).astype(np.float64)
    assert np.abs(centre - want["pts_center"]).max() <= 1e-6 * np.abs(want["pts_center"]).max()
    assert torch.equal(got["zero_mean_pts"], got["pts"] - got["pts_center"].unsqueeze(1))
    # every sampled pixel is one of the object's: a positive depth within max_depth
    assert (pts[..., 2] > 0).all() and (pts[..., 2] <= 4.0).all()


def test_inputs_on_the_device_and_as_tensors_give_the_same_batch():
    from genpose2_amd.frontend import InferDataset, frame_objects
    depth, color, mask = (a.copy() for a in frame())
    want = device_batch((ID_A, ID_B, ID_C), 56, 128)
    got = frame_objects(torch.from_numpy(depth).to(DEV), torch.from_numpy(color), torch.from_numpy(mask).to(DEV),
                        {"camera": {"intrinsics": INTR}}, img_size=56, n_pts=128, seed=SEED, device=DEV)
    ds = InferDataset({"depth": depth, "color": color, "mask": mask, "meta": INTR}, img_size=56, device=DEV, n_pts=128)
    ds.seed = SEED
    got2 = ds.get_objects()
    for k in ("pts", "roi_xs", "roi_ys", "roi_rgb", "count", "pts_center"):
        assert torch.equal(got[k], want[k]) and torch.equal(got2[k], want[k]), k
    # the inputs are not modified (the reference zeroes depth beyond max_depth in place)
    assert all(np.array_equal(a, b) for a, b in zip((depth, color, mask), frame()))


def test_seeds_and_sampling():
    objects, S, n = (ID_A, ID_B, ID_C), 56, 128
    one = device_batch(objects, S, n)
    from genpose2_amd.frontend import frame_objects
    depth, color, mask = frame(objects)
    again = frame_objects(depth, color, mask, INTR, img_size=S, n_pts=n, seed=SEED, device=DEV)
    for k in ("pts", "roi_xs", "roi_ys", "roi_rgb", "count", "pts_center"):
        assert torch.equal(one[k], again[k]), k
    other = device_batch(objects, S, n, SEED + 1)
    a, b = sorted(objects).index(ID_A), sorted(objects).index(ID_B)
    assert not torch.equal(one["roi_xs"][a], other["roi_xs"][a]) or not torch.equal(one["roi_ys"][a], other["roi_ys"][a])
    for k in ("pts", "roi_xs", "roi_ys"):
        assert torch.equal(one[k][b], other[k][b]), k             # tiling draws nothing
    want = expected(objects, S, n, SEED + 1)
    assert np.array_equal(_np(other["roi_xs"]), want["roi_xs"]) and np.array_equal(_np(other["roi_ys"]), want["roi_ys"])
    lin = _np(one["roi_xs"][a]).astype(np.int64) * S + _np(one["roi_ys"][a])
    assert len(np.unique(lin)) == n                               # A's sample is without repetition
    # a 64-bit seed: the high half keys the sample too
    hi = device_batch(objects, S, n, SEED + (1 << 32))
    want = expected(objects, S, n, SEED + (1 << 32))
    assert np.array_equal(_np(hi["roi_xs"]), want["roi_xs"]) and not torch.equal(hi["roi_xs"][a], one["roi_xs"][a])


def test_sample_does_not_depend_on_the_other_objects():
    alone, both = device_batch((ID_A,), 56, 128), device_batch((ID_A, ID_B), 56, 128)
    assert _np(both["ids"]).tolist() == [ID_A, ID_B]
    for k in ("pts", "roi_xs", "roi_ys", "roi_rgb", "count", "pts_center"):
        assert torch.equal(alone[k][0], both[k][0]), k


def test_selection_of_every_valid_pixel_and_of_all_but_one():
    """c == n_pts (a permutation of V) and c == n_pts + 1: the thresholds of the selection path."""
    from genpose2_amd.frontend import frame_objects
    depth, color, mask = frame((ID_B,))
    c = int(expected((ID_B,), 56, 16)["count"][0])
    assert 16 < c <= 2048
    for n in (c, c - 1, c + 1):
        want = ref.frame_objects(depth, color, mask, INTR, 56, n, 4.0, 5)
        got = frame_objects(depth, color, mask, INTR, img_size=56, n_pts=n, seed=5, device=DEV)
        assert np.array_equal(_np(got["roi_xs"]), want["roi_xs"]) and np.array_equal(_np(got["roi_ys"]), want["roi_ys"])
        assert np.array_equal(_np(got["pts"]), want["pts"])


@pytest.mark.parametrize("objects,S,n_pts", CASES)
def test_roi_rgb(objects, S, n_pts):
    _, color, _ = frame(objects)
    want = expected(objects, S, n_pts)
    got = _np(device_batch(objects, S, n_pts)["roi_rgb"])
    assert got.shape == (len(objects), 3, S, S) and got.dtype == np.float32
    mean, std = np.array(ref.MEAN)[:, None, None], np.array(ref.STD)[:, None, None]
    skipped = total = 0
    for b, box in enumerate(want["boxes"]):
        norm, level, dist = ref.roi_rgb(color, box, S)
        keep = (dist > 1e-3).transpose(2, 0, 1)
        skipped += int((~keep).sum())
        total += keep.size
        got_level = np.rint(((got[b].astype(np.float64) * std) + mean) * 255.0)
        assert np.array_equal(got_level[keep], level.transpose(2, 0, 1)[keep].astype(np.float64))
        assert np.abs(got[b].astype(np.float64) - norm)[keep].max() <= 1e-6
        assert level.max() > 0
    print(f"roi_rgb S={S}: {skipped} of {total} values within 1e-3 of a rounding boundary")
    assert skipped <= 0.01 * total


def test_too_few_valid_points_names_the_object():
    from genpose2_amd.frontend import frame_objects
    depth, color, mask = frame((ID_A, ID_B, ID_C, ID_D))
    with pytest.raises(ValueError, match=rf"\b{ID_D}\b"):
        frame_objects(depth, color, mask, INTR, img_size=56, n_pts=128, seed=SEED, device=DEV)
    with pytest.raises(ValueError, match=f"object {ID_D}"):
        ref.frame_objects(depth, color, mask, INTR, 56, 128, 4.0, SEED)
    # no valid pixel at all: B without depth
    depth, color, mask = frame((ID_A, ID_B))
    depth = depth.copy()
    depth[mask == ID_B] = 0
    with pytest.raises(ValueError, match=rf"id {ID_B} has 0 valid"):
        frame_objects(depth, color, mask, INTR, img_size=56, n_pts=128, seed=SEED, device=DEV)


def test_frame_without_objects():
    from genpose2_amd.frontend import frame_objects
    depth, color, mask = frame(())
    out = frame_objects(depth, color, mask, INTR, img_size=56, n_pts=128, device=DEV)
    assert out["pts"].shape == (0, 128, 3) and out["roi_rgb"].shape == (0, 3, 56, 56) and out["ids"].numel() == 0


# ---------------------------------------------------------------------------- GenPose2.inference
K_CAND = 20


def _cfg():
    from genpose2_amd.infer import default_config
    return default_config(device=DEV, sampling_steps=5, eval_repeat_num=K_CAND, noise_seed=3)


def _prev_pose(batch):
    B = batch["pts"].shape[0]
    g = torch.Generator().manual_seed(8)
    q = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)
    from genpose2_amd.aggregate import quaternion_to_matrix
    prev = torch.eye(4).repeat(B, 1, 1)
    prev[:, :3, :3] = quaternion_to_matrix(q)
    prev[:, :3, 3] = batch["pts_center"].cpu() + 0.01 * torch.randn(B, 3, generator=g)
    return prev


def _by_hand(batch, init_x, T0):
    """The EvaluationPipeline's stages one after the other, with fresh agents of the same seeds."""
    from genpose2_amd import aggregate, device as dev
    from genpose2_amd.infer import GenPose2
    gp = GenPose2(None, cfg=_cfg())
    cfg = gp.cfg
    torch.manual_seed(21)
    data = dict(batch)
    pred_pose, _ = gp.score_agent.pred_func(data=data, repeat_num=cfg.eval_repeat_num, T0=T0, init_x=init_x,
                                            return_average_res=False, return_process=False)
    energy = gp.energy_agent.get_energy(data=dict(batch), pose_samples=pred_pose, T=None, mode="test",
                                        extract_feature=True)
    agg = aggregate.aggregate_pose(pred_pose, energy, cfg.retain_ratio, cfg.clustering, cfg.clustering_eps,
                                   cfg.clustering_minpts, retain_num=int(cfg.eval_repeat_num * cfg.retain_ratio))
    return agg, dev.bbox_length(batch["pts"], agg)


@pytest.mark.parametrize("warm,tracking", [(False, False), (True, True), (True, False)])
def test_genpose2_inference_equals_stages_by_hand(warm, tracking):
    from genpose2_amd.infer import GenPose2, create_genpose2, pose_representation
    batch = device_batch((ID_A, ID_B, ID_C), 56, 1024)
    B = batch["pts"].shape[0]
    prev = _prev_pose(batch) if warm else None
    gp = create_genpose2(None, None, None, _cfg())
    assert gp.cfg.sampler_mode == ["ode"] and gp.cfg.T0 == 0.55 and gp.scale_agent is None
    torch.manual_seed(21)
    pose, length = gp.inference(batch, prev_pose=prev, tracking=tracking, tracking_T0=0.15)
    assert pose.shape == (B, 4, 4) and length.shape == (B, 3)
    assert torch.isfinite(pose).all() and torch.isfinite(length).all() and (length > 0).all()
    R = pose[:, :3, :3].double()
    assert (R @ R.transpose(1, 2) - torch.eye(3, device=R.device, dtype=R.dtype)).abs().max() < 1e-5
    assert torch.equal(pose[:, 3], torch.tensor([0., 0., 0., 1.], device=pose.device).repeat(B, 1))

    init_x = None
    if warm:
        init_x = pose_representation(prev.to(DEV))
        assert torch.equal(init_x[:, :3], prev[:, :3, 0].to(DEV)) and torch.equal(init_x[:, 3:6], prev[:, :3, 1].to(DEV))
        init_x[:, 6:] -= batch["pts_center"]
    want_pose, want_length = _by_hand(batch, init_x, 0.15 if (warm and tracking) else 0.55)
    assert torch.equal(pose, want_pose) and torch.equal(length, want_length)
    if warm:   # the start time matters: the other tracking flag gives another result
        other, _ = _by_hand(batch, init_x, 0.55 if tracking else 0.15)
        assert not torch.equal(other, pose)


def test_genpose2_inference_takes_an_infer_dataset_and_a_pose_list():
    from genpose2_amd.frontend import InferDataset
    from genpose2_amd.infer import GenPose2
    depth, color, mask = frame()
    ds = InferDataset({"depth": depth, "color": color, "mask": mask, "meta": {"camera": {"intrinsics": INTR}}},
                      img_size=56, device=DEV)
    ds.seed = SEED
    batch = device_batch((ID_A, ID_B, ID_C), 56, 1024)
    prev = _prev_pose(batch)
    torch.manual_seed(21)
    a = GenPose2(None, cfg=_cfg()).inference(ds, prev_pose=[prev], tracking=True)
    torch.manual_seed(21)
    b = GenPose2(None, cfg=_cfg()).inference(batch, prev_pose=prev.to(DEV), tracking=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="prev_pose"):
        GenPose2(None, cfg=_cfg()).inference(batch, prev_pose=prev[:1])


def test_genpose2_loads_checkpoints_and_sizes_with_the_scalenet(tmp_path):
    from conftest import write_reference_checkpoint
    from genpose2_amd.infer import GenPose2
    paths = [write_reference_checkpoint(str(tmp_path / f"{kind}.pth"), kind, seed=1)
             for kind in ("score", "energy", "scale")]
    batch = device_batch((ID_A, ID_B, ID_C), 56, 1024)
    gp = GenPose2(*paths, cfg=_cfg())
    assert [a.weights_source for a in (gp.score_agent, gp.energy_agent, gp.scale_agent)] == paths
    torch.manual_seed(21)
    pose, length = gp.inference(batch)
    assert pose.shape == (3, 4, 4) and length.shape == (3, 3) and torch.isfinite(length).all()
    data = dict(batch)
    gp.score_agent.encode_func(data)
    _, want = gp.scale_agent.pred_scale_func({"pts_feat": data["pts_feat"], "rgb_feat": None,
                                              "axes": pose[:, :3, :3].contiguous()})
    assert torch.equal(length, want)
    torch.manual_seed(21)
    other, _ = GenPose2(None, cfg=_cfg()).inference(batch)      # the synthetic weights of seed 0
    assert not torch.equal(other, pose)
