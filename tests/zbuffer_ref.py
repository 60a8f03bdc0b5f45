"""The mesh z-buffer of include/csplat.h (csplat_zb_mesh, csplat_zb_points, csplat_zb_mark) restated in numpy, face by face.

Coverage is int64 arithmetic on the snapped coordinates: exact, compared for equality.  The depth comes twice: in float64 from the snapped
integers and the float32 1 / z of the screen records (the yardstick), and as a float32 restatement of the header's operations (what gives the
project's bar: 8 x its own error against float64, floor 1e-6).  Stage P likewise: float32 as the header states it, and float64."""
import numpy as np

SUB = 256
GUARD = 16384.0
K_BAR, FLOOR = 8.0, 1e-6          # the rule of tests/test_train_kernels_gpu.py


def project(vertices, intr, w2c, near=0.01, dtype=np.float32):
    """stage P: vertices [N,3] or [V,N,3], intr [V,4], w2c [V,3,4] -> dict(px, py, z, iz, valid [V,N]; screen [V,N,4] int32)"""
    intr, w2c = np.asarray(intr, np.float32).astype(dtype), np.asarray(w2c, np.float32)[:, :3].astype(dtype)
    V = intr.shape[0]
    P = np.asarray(vertices, np.float32).astype(dtype)
    P = np.broadcast_to(P, (V,) + P.shape[-2:])
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    r = lambda i, j: w2c[:, i, j, None]  # noqa: E731
    with np.errstate(all="ignore"):
        x = r(0, 0) * X + r(0, 1) * Y + r(0, 2) * Z + r(0, 3)
        y = r(1, 0) * X + r(1, 1) * Y + r(1, 2) * Z + r(1, 3)
        z = r(2, 0) * X + r(2, 1) * Y + r(2, 2) * Z + r(2, 3)
        px = (intr[:, 0, None] * x) / z + intr[:, 2, None]
        py = (intr[:, 1, None] * y) / z + intr[:, 3, None]
        iz = dtype(1) / z
        valid = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(px) & np.isfinite(py) & np.isfinite(iz)
        valid &= (z > dtype(np.float32(near))) & (np.abs(px) <= GUARD) & (np.abs(py) <= GUARD)
        sx = np.rint(dtype(SUB) * np.where(valid, px, 0)).astype(np.int32)
        sy = np.rint(dtype(SUB) * np.where(valid, py, 0)).astype(np.int32)
    bits = np.where(valid, iz, 0).astype(np.float32).view(np.int32)
    return dict(px=px, py=py, z=z, iz=iz, valid=valid, screen=np.stack([sx, sy, bits, valid.astype(np.int32)], -1))


def owns(E, dx, dy):
    return (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def stage_d(c, Px, Py):
    """corner records c [...,3,4] (int) at snapped points Px, Py (int64, broadcasting against c[..., 0, 0]) -> dict(cov; z64, z32; t64, t32:
    the perspective-correct weights [3] in the face's own corner order)"""
    c = c.astype(np.int64)
    x0, y0, x1, y1, x2, y2 = c[..., 0, 0], c[..., 0, 1], c[..., 1, 0], c[..., 1, 1], c[..., 2, 0], c[..., 2, 1]
    A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    live = (c[..., 0, 3] != 0) & (c[..., 1, 3] != 0) & (c[..., 2, 3] != 0) & (A != 0)
    sw = A < 0
    x1, x2, y1, y2 = np.where(sw, x2, x1), np.where(sw, x1, x2), np.where(sw, y2, y1), np.where(sw, y1, y2)
    A = np.abs(A)
    E01 = (x1 - x0) * (Py - y0) - (y1 - y0) * (Px - x0)
    E12 = (x2 - x1) * (Py - y1) - (y2 - y1) * (Px - x1)
    E20 = (x0 - x2) * (Py - y2) - (y0 - y2) * (Px - x2)
    cov = live & owns(E01, x1 - x0, y1 - y0) & owns(E12, x2 - x1, y2 - y1) & owns(E20, x0 - x2, y0 - y2)
    assert np.all((E01 + E12 + E20 == A) | ~live)                      # the three weights sum to the area
    iz = [c[..., k, 2].astype(np.int32).view(np.float32) for k in range(3)]
    out = dict(cov=cov)
    with np.errstate(all="ignore"):
        for dt, tag in ((np.float64, "64"), (np.float32, "32")):
            fA = A.astype(dt)
            w0, w1, w2 = E12.astype(dt) / fA, E20.astype(dt) / fA, E01.astype(dt) / fA
            b = (w0, np.where(sw, w2, w1), np.where(sw, w1, w2))
            q = b[0] * iz[0].astype(dt) + b[1] * iz[1].astype(dt) + b[2] * iz[2].astype(dt)
            out["z" + tag] = dt(1) / q
            out["t" + tag] = [(b[i] * iz[i].astype(dt)) / q for i in range(3)]
    return out


def raster(screen, faces, H, W):
    """every face of every view, in ascending face index, over the pixels of its bounding box ->
      count [V,H,W]   the number of faces that cover the pixel
      z64, face64     the smallest float64 depth (inf: none) and its face (-1); second64: the runner-up's depth (inf: none)
      z32, face32     the float32 restatement: the winner by the key (float bits of z) << 32 | face
      t64, t32        [V,3,H,W] the perspective-correct weights of face64 / face32, 0 on the background"""
    screen, faces = np.asarray(screen), np.asarray(faces, np.int64).reshape(-1, 3)
    V = screen.shape[0]
    count = np.zeros((V, H, W), np.int32)
    z64, second64 = np.full((V, H, W), np.inf), np.full((V, H, W), np.inf)
    face64 = np.full((V, H, W), -1, np.int32)
    key32 = np.full((V, H, W), np.iinfo(np.uint64).max, np.uint64)
    t64, t32 = np.zeros((V, 3, H, W)), np.zeros((V, 3, H, W), np.float32)
    for v in range(V):
        for f, tri in enumerate(faces):
            c = screen[v][tri]
            if not c[:, 3].all():
                continue
            X0, X1 = max(0, -(-int(c[:, 0].min()) // SUB)), min(W - 1, int(c[:, 0].max()) // SUB)
            Y0, Y1 = max(0, -(-int(c[:, 1].min()) // SUB)), min(H - 1, int(c[:, 1].max()) // SUB)
            if X0 > X1 or Y0 > Y1:
                continue
            Px = SUB * np.arange(X0, X1 + 1, dtype=np.int64)[None, :]
            Py = SUB * np.arange(Y0, Y1 + 1, dtype=np.int64)[:, None]
            d = stage_d(c, Px, Py)
            cov = d["cov"]
            if not cov.any():
                continue
            box = (v, slice(Y0, Y1 + 1), slice(X0, X1 + 1))
            count[box] += cov
            zf = np.where(cov, d["z64"], np.inf)
            best, sec = z64[box], second64[box]
            wins = zf < best
            second64[box] = np.where(wins, best, np.minimum(sec, zf))
            z64[box] = np.where(wins, zf, best)
            face64[box] = np.where(wins, f, face64[box])
            key = (d["z32"].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            take = cov & (key < key32[box])
            key32[box] = np.where(take, key, key32[box])
            for i in range(3):
                t64[(v, i) + box[1:]] = np.where(wins, d["t64"][i], t64[(v, i) + box[1:]])
                t32[(v, i) + box[1:]] = np.where(take, d["t32"][i], t32[(v, i) + box[1:]])
    hit = key32 != np.iinfo(np.uint64).max
    z32 = np.where(hit, (key32 >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf)).astype(np.float32)
    face32 = np.where(hit, (key32 & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return dict(count=count, z64=z64, second64=second64, face64=face64, z32=z32, face32=face32, t64=t64, t32=t32)


def at_faces(screen, faces, ids):
    """the face ids [V,H,W] of somebody else's image -> (covered [V,H,W] by the integer rule, that face's float64 depth there)"""
    screen, faces, ids = np.asarray(screen), np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(ids)
    V, H, W = ids.shape
    Px = SUB * np.arange(W, dtype=np.int64)[None, :]
    Py = SUB * np.arange(H, dtype=np.int64)[:, None]
    cov, z = np.zeros((V, H, W), bool), np.full((V, H, W), np.inf)
    for v in range(V):
        d = stage_d(screen[v][faces[np.maximum(ids[v], 0)]], Px, Py)
        cov[v], z[v] = d["cov"] & (ids[v] >= 0), d["z64"]
    return cov, z


def ray_factor(intr, H, W, dtype):
    intr = np.asarray(intr, np.float32).astype(dtype)
    u = (np.arange(W, dtype=dtype)[None, None, :] - intr[:, 2, None, None]) / intr[:, 0, None, None]
    w = (np.arange(H, dtype=dtype)[None, :, None] - intr[:, 3, None, None]) / intr[:, 1, None, None]
    return np.sqrt(u * u + w * w + dtype(1))


def depth_image(z, intr, kind, dtype):
    """z [V,H,W] with inf on the background -> the depth image of `kind` in `dtype`, 0 on the background"""
    hit = np.isfinite(z)
    d = np.where(hit, z, 0).astype(dtype)
    if kind == "ray":
        d = d * ray_factor(intr, z.shape[1], z.shape[2], dtype)
    return np.where(hit, d, 0).astype(dtype)


def depth_bar(r32, r64, unit=1.0):
    """the absolute bar of check() for these two images: max(8 e32, 1e-6) x the scale"""
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64, np.float64)
    scale = max(float(np.abs(r64).max()) if r64.size else 0.0, unit)
    return max(K_BAR * float(np.abs(r32 - r64).max() if r64.size else 0.0) / scale, FLOOR) * scale


def points(pts, intr, w2c, H, W, near=0.01):
    """points as one-pixel primitives, the float32 restatement -> (z [V,H,W] float32 with inf where no point lands, point_id [V,H,W])"""
    p = project(pts, intr, w2c, near)
    V, M = p["valid"].shape
    z = np.full((V, H, W), np.inf, np.float32)
    ids = np.full((V, H, W), -1, np.int32)
    with np.errstate(all="ignore"):
        rx, ry = np.rint(p["px"]), np.rint(p["py"])
    for v in range(V):
        for m in range(M):
            if not p["valid"][v, m] or not (0 <= rx[v, m] <= W - 1 and 0 <= ry[v, m] <= H - 1):
                continue
            x, y = int(rx[v, m]), int(ry[v, m])
            if p["z"][v, m] < z[v, y, x]:          # ascending m: an equal depth keeps the lower index
                z[v, y, x], ids[v, y, x] = p["z"][v, m], m
    return z, ids


def visibility(face_id, faces, N):
    face_id, faces = np.asarray(face_id), np.asarray(faces, np.int64).reshape(-1, 3)
    V = face_id.shape[0]
    fv, nv = np.zeros((V, len(faces)), bool), np.zeros((V, N), bool)
    for v in range(V):
        seen = np.unique(face_id[v][face_id[v] >= 0])
        fv[v, seen] = True
        nv[v, faces[seen].reshape(-1)] = True
    return fv, nv


def grid_faces(g, rng=None):
    """the two triangles of every cell of a g x g vertex grid (vertex j * g + i); with `rng`, every face's winding and first corner at random"""
    faces = []
    for j in range(g - 1):
        for i in range(g - 1):
            a, b, c, d = j * g + i, j * g + i + 1, (j + 1) * g + i, (j + 1) * g + i + 1
            faces += [[a, b, d], [a, d, c]]
    faces = np.array(faces, np.int64)
    if rng is not None:
        for k in range(len(faces)):
            faces[k] = np.roll(faces[k], int(rng.integers(0, 3)))
            if rng.integers(0, 2):
                faces[k] = faces[k][::-1]
    return faces


# ---------------------------------------------------------------------------------------------------------------- dyadic fixtures
# R = I, t = 0, fx = fy = 16, cx and cy multiples of 1/4, pixel coordinates multiples of 1/4 and z a power of two: x = (p - cx) z / 16 is a
# multiple of 2^-14, and fx * x, / z and + cx are all exact in float32 -- stage P is exact with or without fused multiply-adds
DYADIC_F = 16.0
EYE34 = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]], np.float32)


def dyadic_camera(H, W, V=1):
    intr = np.array([[DYADIC_F, DYADIC_F, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.25]] * V, np.float32)
    return intr, np.repeat(EYE34[None], V, 0)


def unproject_pixels(pix, z, intr1):
    """pixel coordinates [...,2] and depths [...] under one dyadic camera (fx, fy, cx, cy) -> camera-space points [...,3] float32, exact"""
    pix, z = np.asarray(pix, np.float64), np.asarray(z, np.float64)
    out = np.stack([(pix[..., 0] - intr1[2]) * z / intr1[0], (pix[..., 1] - intr1[3]) * z / intr1[1], z], -1)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


def soup(rng, F, H, W, intr1, extent=6.0, margin=6.0):
    """F small triangles with corners on multiples of 1/4 pixel (a sixteenth of them on pixel centres, many edges through centres) around
    and beyond the image, z in {1, 2, 4} per corner -> (vertices [3F,3], faces [F,3])"""
    centre = np.stack([rng.uniform(-margin, W - 1 + margin, F), rng.uniform(-margin, H - 1 + margin, F)], -1)
    pix = np.round((centre[:, None, :] + rng.uniform(-extent, extent, (F, 3, 2))) * 4) / 4
    z = rng.choice(np.array([1.0, 2.0, 4.0]), (F, 3))
    return unproject_pixels(pix, z, intr1).reshape(-1, 3), np.arange(3 * F, dtype=np.int64).reshape(F, 3)


def special(H, W, intr1):
    """the faces a draw can go wrong at -> (vertices, faces, names): off the image on each side, cut by each border, no area, a repeated
    corner, a corner behind `near`, a corner beyond the guard, both windings, corners on pixel centres, edges through centres"""
    w, h = float(W - 1), float(H - 1)
    tris = [("off left", [(-9, 2), (-3, 2), (-6, 7)], 2), ("off right", [(w + 3, 2), (w + 9, 2), (w + 6, 7)], 2),
            ("off top", [(2, -9), (7, -9), (4, -2)], 2), ("off bottom", [(2, h + 2), (7, h + 2), (4, h + 9)], 2),
            ("cut left", [(-4, 1), (5, 3), (-2, 9)], 2), ("cut right", [(w - 5, 1), (w + 6, 4), (w - 3, 9)], 2),
            ("cut top", [(8, -5), (16, -3), (11, 5)], 4), ("cut bottom", [(8, h - 4), (16, h - 2), (11, h + 6)], 4),
            ("no area", [(3, 3), (6, 6), (9, 9)], 1), ("ccw", [(10, 10), (20, 12), (12, 20)], 1), ("cw", [(10, 10), (12, 20), (20, 12)], 2),
            ("centres", [(4, 12), (12, 12), (4, 20)], 1), ("through centres", [(14.5, 2.5), (24.5, 12.5), (14.5, 12.5)], 1),
            ("whole image", [(-3, -3), (2 * w + 9, -3), (-3, 2 * h + 9)], 4)]
    pix = np.array([t[1] for t in tris], np.float64)
    z = np.array([[t[2]] * 3 for t in tris], np.float64)
    z[9] = [1, 2, 4]                                                                              # a tilted face
    verts = unproject_pixels(pix, z, intr1).reshape(-1, 3)
    faces = np.arange(len(verts), dtype=np.int64).reshape(-1, 3)
    names = [t[0] for t in tris]
    behind = unproject_pixels(np.array([[5.0, 5.0]]), np.array([2.0 ** -8]), intr1)                # z = 1/256 < near = 0.01
    beyond = unproject_pixels(np.array([[20000.0, 5.0]]), np.array([1.0]), intr1)                  # |px| > 16384
    n = len(verts)
    verts = np.concatenate([verts, behind, beyond])
    faces = np.concatenate([faces, [[27, 27, 28], [27, 28, n], [27, 28, n + 1]]])                  # (27, 28: corners of the "ccw" face)
    return verts, faces, names + ["repeated corner", "behind near", "beyond the guard"]


def folded_grid(g, H, W, intr1, rng):
    """a g x g grid folded twice along x, so that 2-3 layers overlap at z = 1, 2, 4 (random windings), and one face twice (the copy last)"""
    i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="xy")
    t = i / (g - 1) * 3.0                                                                          # three panels: right, back left, right again
    fold = np.where(t <= 1, t, np.where(t <= 2, 2 - t, t - 2))
    pix = np.stack([np.round((2 + fold * (W - 5)) * 4) / 4, np.round((2 + j / (g - 1) * (H - 5)) * 4) / 4], -1)
    z = np.where(t <= 1, 4.0, np.where(t <= 2, 2.0, 1.0))
    verts = unproject_pixels(pix.reshape(-1, 2), z.reshape(-1), intr1)
    faces = grid_faces(g, rng)
    return verts, np.concatenate([faces, np.roll(faces[-1], 1)[None]])                     # (the last face: on the front panel)
