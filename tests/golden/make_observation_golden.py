"""Generates tests/golden/observation.npz: one small observation scene with the outputs of the reference's OWN functions.

Run ONLY where the reference checkout exists (CSPLAT_REFERENCE, default /root/reference); the tests read the .npz alone.  As
tests/golden/make_tracking_golden.py does, the functions are exec'd at generation time from the reference's text: its modules do not
import here (their simulator dependencies are absent).  `intrinsic_from_fov` and `get_world_coords` come from manipulation/deform_mesh.py
(:94-111, :168-195: the form that takes the world-to-camera matrix; the twin in manipulation/envs/camera_utils.py:106-133 builds it from a
simulator environment), `get_observable_particle_index` and `_old` from manipulation/envs/camera_utils.py:136-162.  No reference text is
stored: the fixture holds the inputs, the reference's world coordinates and its observable particle sets.

The scene: 2 views of 40 x 30 pixels looking down on a 25 x 12 particle grid; the depth images are the z-depth of the plane under the
grid plus noise, with about a third of the pixels holes (0 or negative -- the reference selects `depth > 0`).  Ties: the observable sets
are decisions on distances.  A cloud point whose k-th and (k+1)-th nearest particle are closer in squared distance than MARGIN (k = 1
and k = 2) gets its depth redrawn until none is left, so that float32 and float64 arithmetic must reach the same sets: MARGIN is 64 x the
float32 rounding (2^-23) of the largest squared distance of the scene."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import scipy.spatial

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "cloth-splatting_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
REF = os.environ.get("CSPLAT_REFERENCE", "/root/reference")

V, W, H = 2, 40, 30
GRID = (25, 12)
FOV_DEG = 45.0          # get_world_coords of deform_mesh.py calls intrinsic_from_fov(height, width, 45)
NOISE, HOLES = 0.01, 1.0 / 3.0


def reference_functions(path, names):
    """the named top-level functions of a reference file, exec'd on the CPU -> namespace"""
    src = open(os.path.join(REF, path)).read()
    ns = dict(np=np, scipy=scipy)
    for name in names:
        m = re.search(r"^def " + name + r"\(.*?(?=^\S|\Z)", src, re.S | re.M)
        assert m, (path, name)
        exec(compile(m.group(0), f"{path}:{name}", "exec"), ns)
    return SimpleNamespace(**{n: ns[n] for n in names})


def margin_of(cloud, particles):
    import observation_ref as R
    return 64.0 * 2.0 ** -23 * float(R.sq_dists(cloud, particles, np.float64).max())


def main():
    import observation_ref as R
    from csplat import synthetic as syn
    assert os.path.isdir(REF), "the fixture can only be generated where the reference checkout exists"
    dm = reference_functions("manipulation/deform_mesh.py", ["intrinsic_from_fov", "get_world_coords"])
    cu = reference_functions("manipulation/envs/camera_utils.py", ["get_observable_particle_index", "get_observable_particle_index_old"])
    rng = np.random.default_rng(20241019)
    gx, gy = np.meshgrid(np.linspace(-1.2, 1.2, GRID[0]), np.linspace(-0.55, 0.55, GRID[1]), indexing="xy")
    particles = np.stack([gx, gy, 0.03 * np.sin(3 * gx) * np.cos(2 * gy)], -1).reshape(-1, 3)
    particles = particles.astype(np.float32).astype(np.float64)
    Kref = dm.intrinsic_from_fov(H, W, FOV_DEG)
    intrinsics = np.array([Kref[0, 0], Kref[1, 1], Kref[0, 2], Kref[1, 2]], np.float64)
    rgb = np.zeros((H, W, 3), np.float32)
    w2c, depth = [], np.zeros((V, H, W), np.float32)
    for v, theta in enumerate((20.0, -35.0)):
        cam = syn.make_camera(theta, W, H, phi_deg=-55.0, radius=4.0)
        w2c.append(np.asarray(cam["world_view_transform"], np.float64).T)          # stored transposed: the column-vector form is its transpose
    w2c = np.stack(w2c)
    c2w = np.linalg.inv(w2c)

    def plane_depth(v):
        """the z-depth at which each pixel's ray meets the plane z_world = 0"""
        u, w = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        ray = np.stack([(u - intrinsics[2]) / intrinsics[0], (w - intrinsics[3]) / intrinsics[1], np.ones_like(u)], -1)
        dz = ray @ c2w[v, 2, :3]
        return -c2w[v, 2, 3] / dz

    base = np.stack([plane_depth(v) for v in range(V)])
    assert (base > 1.0).all() and (base < 20.0).all(), (base.min(), base.max())
    depth[:] = (base + rng.normal(0.0, NOISE, base.shape)).astype(np.float32)
    hole = rng.random((V, H, W)) < HOLES
    depth[hole] = np.where(rng.random(int(hole.sum())) < 0.5, 0.0, -1.0).astype(np.float32)

    redrawn = 0
    while True:
        world = np.stack([dm.get_world_coords(rgb, depth[v], w2c[v]) for v in range(V)])[..., :3]
        cloud = world[depth > 0]
        margin = margin_of(cloud, particles)
        bad = np.minimum(R.tie_margins(cloud, particles, 1), R.tie_margins(cloud, particles, 2)) < margin
        if not bad.any():
            break
        at = np.argwhere(depth > 0)[bad]
        for v, y, x in at:
            depth[v, y, x] = np.float32(base[v, y, x] + rng.normal(0.0, NOISE))
        redrawn += len(at)
        assert redrawn < 10000
    obs2 = np.zeros((V, len(particles)), bool)
    obs1 = np.zeros((V, len(particles)), bool)
    for v in range(V):
        i2 = cu.get_observable_particle_index(world[v], particles, rgb, depth[v])
        i1 = cu.get_observable_particle_index_old(world[v], particles, rgb, depth[v])
        assert i2.dtype == np.int32 and i1.dtype == np.int32
        obs2[v, i2] = True
        obs1[v, i1] = True
    out = os.path.join(HERE, "observation.npz")
    np.savez_compressed(out, depth=depth, world=world, world_to_camera=w2c, intrinsics=intrinsics, particles=particles.astype(np.float32),
                        observable_k2=obs2, observable_k1=obs1, margin=np.float64(margin), redrawn=np.int64(redrawn))
    print(f"wrote {out}: {os.path.getsize(out)} bytes; {int((depth > 0).sum())} of {depth.size} pixels valid, {redrawn} redrawn, "
          f"margin {margin:.3e}, observable {obs2.sum(1).tolist()} (k=2) {obs1.sum(1).tolist()} (k=1) of {len(particles)}")


if __name__ == "__main__":
    main()
