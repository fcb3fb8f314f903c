"""NumPy restatement of the pose hypotheses (gp_rank_aggregate_modes) for arbitrary inputs.

It follows oracle.aggregate_pose statement by statement (oracle.sort_poses_by_energy, oracle.rot6_to_matrix,
oracle.matrix_to_quaternion, sklearn's DBSCAN on the float32 distance matrix, oracle.average_quaternion_batch) and
keeps what that function drops: the labels, and every cluster's average instead of the largest one's. It is pinned
to the reference by tests/golden/golden_modes.npz (tests/test_cpu_modes.py).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from oracle import oracle


def row_margin(D: np.ndarray, eps: float) -> float:
    """min over pairs of | ||D_i - D_j||_2 - eps | / eps: how far the labels are from depending on rounding."""
    X = D.astype(np.float64)
    rd = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    return float(np.abs(rd - eps).min() / eps)


def prev_quaternion(prev_rot: np.ndarray) -> np.ndarray:
    """(B,3,3) -> (B,4): the quaternion of the rotation rebuilt from its first two columns."""
    rot6 = np.concatenate([prev_rot[:, :, 0], prev_rot[:, :, 1]], -1).astype(np.float32)
    return oracle.matrix_to_quaternion(oracle.rot6_to_matrix(rot6))


def modes_ref(pred_pose: np.ndarray, pred_energy: np.ndarray, keep: int, clustering: int, eps: float,
              min_samples: int, max_modes: int, prev_rot: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    from sklearn.cluster import DBSCAN
    bs, K = pred_pose.shape[:2]
    M = max_modes
    sp, _, o_rot, _ = oracle.sort_poses_by_energy(pred_pose, pred_energy)
    good = sp[:, :keep]
    own = np.take_along_axis(pred_pose, o_rot[:, :keep, None], 1)             # rank r's own candidate, all 9
    own_e = np.take_along_axis(pred_energy[..., 0], o_rot[:, :keep], 1)
    q = oracle.matrix_to_quaternion(oracle.rot6_to_matrix(good[:, :, :6].reshape(bs * keep, -1))).reshape(bs, keep, 4)
    qa = oracle.average_quaternion_batch(q)
    out = dict(labels=np.full((bs, keep), -1, np.int64), slot_label=np.full((bs, M), -1, np.int64),
               mode_pose=np.zeros((bs, M, 4, 4), np.float32), mode_quat=np.zeros((bs, M, 4), np.float32),
               mode_count=np.zeros((bs, M), np.int32), mode_energy=np.zeros((bs, M), np.float32),
               mode_spread=np.zeros((bs, M), np.float32), n_clusters=np.zeros(bs, np.int32),
               noise_count=np.zeros(bs, np.int32), nearest=np.full(bs, -1, np.int32),
               margin=np.full(bs, np.inf), nearest_gap=np.full(bs, np.inf))
    qp = prev_quaternion(prev_rot) if prev_rot is not None else None
    for j in range(bs):
        order = [None]                       # no cluster: the whole kept set
        if clustering:
            D = (1 - (q[j][None] * q[j][:, None]).sum(2) ** 2).astype(np.float32)
            labels = DBSCAN(eps=eps, min_samples=min_samples).fit(D).labels_
            out["labels"][j] = labels
            out["margin"][j] = row_margin(D, eps)
            L = int(labels.max()) + 1
            out["n_clusters"][j], out["noise_count"][j] = L, int((labels == -1).sum())
            if L > 0:
                bins = np.bincount(labels[labels >= 0])
                order = sorted(range(L), key=lambda l: (-bins[l], l))
                assert order[0] == int(np.argmax(bins))
        for m, l in enumerate(order[:M]):
            member = labels == l if l is not None else np.ones(keep, bool)
            qm = oracle.average_quaternion_batch(q[j, member][None])[0]
            if m == 0:
                qa[j] = qm
            out["slot_label"][j, m] = -1 if l is None else l
            out["mode_quat"][j, m] = qm
            out["mode_pose"][j, m, :3, :3] = oracle.quaternion_to_matrix(qm)
            out["mode_pose"][j, m, :3, 3] = own[j, member, 6:].mean(0, dtype=np.float32)
            out["mode_pose"][j, m, 3, 3] = 1
            out["mode_count"][j, m] = int(member.sum())
            out["mode_energy"][j, m] = own_e[j, member].mean(dtype=np.float32)
            out["mode_spread"][j, m] = (1 - (q[j, member] * qm).sum(1) ** 2).mean(dtype=np.float32)
        if qp is not None:
            filled = max(1, min(len(order), M))
            d = np.sort((out["mode_quat"][j, :filled].astype(np.float64) * qp[j]).sum(1) ** 2)
            out["nearest"][j] = int(np.argmax((out["mode_quat"][j, :filled] * qp[j]).sum(1) ** 2))
            out["nearest_gap"][j] = d[-1] - d[-2] if filled > 1 else np.inf   # how clear the choice is
    agg = np.zeros((bs, 4, 4), np.float32)
    agg[:, 3, 3] = 1
    agg[:, :3, :3] = oracle.quaternion_to_matrix(qa)
    agg[:, :3, 3] = good[:, :, 6:].mean(1)
    out["aggregated"] = agg
    return out
