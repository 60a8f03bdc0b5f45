"""A numpy / torch-CPU restatement of the camera data set (csplat/camera_dataset.py, csrc/csplat_camera_dataset.hip), written from the
reference's rules (scene_reconstruction/dataset.py:46-123) and from the loader's arithmetic (csplat/scene_io.py): an image is
`uint8 / 255.0` in float32, a mask `1.0 - that`; the grid is ordered by the POSITIONS of the raw ids in their sorted unique lists."""
import numpy as np
import torch

from csplat import synthetic as syn
from csplat.scene_io import CameraInfo


def image_of(levels):
    """float32 image of uint8 levels [..]: one division, as torch's uint8_tensor / 255.0"""
    return torch.from_numpy(np.asarray(levels, np.uint8).astype(np.float32) / np.float32(255.0))


def mask_of(levels):
    """float32 mask of uint8 levels: 1.0 - levels / 255.0, two roundings"""
    return torch.from_numpy(np.float32(1.0) - np.asarray(levels, np.uint8).astype(np.float32) / np.float32(255.0))


def levels(shape, seed):
    """uint8 levels of `shape` = (planes, H, W) in which every plane holds all 256 levels when it has 256 pixels or more (a seeded
    permutation of 0 .. 255 repeated), else a seeded draw"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape[1:]))
    out = np.empty((shape[0], n), np.uint8)
    for p in range(shape[0]):
        reps = -(-n // 256)
        out[p] = np.concatenate([rng.permutation(256) for _ in range(reps)])[:n].astype(np.uint8) if n >= 256 else rng.integers(0, 256, n)
    return out.reshape(shape)


def make_info(view_id, time_id, H, W, mask=True, seed=0, n_times=6, image=None, mask_image=None, uid=None):
    """a CameraInfo as the loader makes it: a seeded 8-bit image (and mask), a camera on a circle, time = time_id / (n_times - 1)"""
    key = seed * 10007 + 101 * view_id + time_id
    img = image_of(levels((3, H, W), key)) if image is None else image
    msk = (mask_of(levels((1, H, W), key + 5003)) if mask_image is None else mask_image) if mask else None
    R, T = syn.c2w_to_RT(syn.pose_spherical(25.0 * view_id - 40.0, -30.0, 4.0))
    focal = W / (2 * np.tan(syn.CAMERA_ANGLE_X / 2))
    return CameraInfo(uid=101 * view_id + time_id if uid is None else uid, R=R, T=T, FovY=float(2 * np.arctan(H / (2 * focal))),
                      FovX=syn.CAMERA_ANGLE_X, image=img, image_path="", image_name=f"r_{view_id}_{time_id}", width=H, height=W,
                      time=time_id / max(n_times - 1, 1), view_id=view_id, time_id=time_id, flow=None, mask=msk)


def grid(infos):
    """(sorted unique view ids, sorted unique time ids, {(view position, time position): info}) -- dataset.py:54-71; of two records of
    one cell the FIRST is kept (add_frames skips cells that are present)"""
    views = sorted({int(i.view_id) for i in infos})
    times = sorted({int(i.time_id) for i in infos})
    cells = {}
    for i in infos:
        cells.setdefault((views.index(int(i.view_id)), times.index(int(i.time_id))), i)
    return views, times, cells


def item_times(n_times, rng):
    """dataset.py:79-85"""
    if n_times >= 3:
        m = int(rng.integers(1, n_times - 1))
        return [m - 1, m, m + 1]
    return list(range(n_times))


def resolve(cells, n_views, view, time, rng):
    """dataset.py:96-107 with the evident intent: the cell's record, else that of a uniformly chosen view that has the time"""
    if (view, time) in cells:
        return cells[(view, time)]
    have = [v for v in range(n_views) if (v, time) in cells]
    if not have:
        raise ValueError("no camera")
    return cells[(have[int(rng.integers(len(have)))], time)]


def driver_sequence(n_views, n_times, static_steps, rounds, rng):
    """the (view, times, static, iteration) of SingleStepOptimizer.static_reconstruction(static_steps) followed by
    update_mesh_predictions(k) for k in rounds (train_utils.py:421-423, :480-496; the triple is (c - 1, c, c + 1), c = draw + 1)"""
    out = [(it % n_views, [0], True, it) for it in range(1, static_steps + 1)]
    last = static_steps
    for k in rounds:
        for it in range(last + 1, last + k + 1):
            if n_times >= 3:
                p = np.linspace(0.5, 1.5, n_times - 2)
                p /= p.sum()
                c = int(rng.choice(n_times - 2, p=p)) + 1
                times = [c - 1, c, c + 1]
            else:
                times = list(range(n_times))
            out.append((it % n_views, times, False, it))
        last += k
    return out
