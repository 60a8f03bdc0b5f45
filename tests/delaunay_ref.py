"""What the Delaunay tests hold the library to (include/csplat.h, "Delaunay triangulation"), in Python integers.  No SciPy except in the
two functions that make and re-derive the fixture.

  (a) exact predicates: the float32 coordinates of a cloud scaled by a common power of two become Python integers; orientation, distance
      comparison and the in-circle determinant with the symbolic tie rule are integer arithmetic
  (b) check(points, faces): is this the triangulation the header defines?  Returns the number of exact ties
  (c) walk(points): the per-point walk with the tie rule -- the prediction of the library's faces, face for face
  (d) threshold_loop: the reference's loop over simplices with its length filter (meshnet/data_utils.py:378-404), restated
  (e) adversarial_records: inputs that sit on and one ulp off the predicates' zero sets, over the whole float32 range
"""
import math
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "delaunay_scipy.npz")
FIXTURE_CLOUDS = ((257, 11), (300, 12), (2048, 13))          # (N, seed)


# ------------------------------------------------------------------------------------------------------------------ (a) exact predicates
def to_ints(points):
    """float32 [N,2] -> list of (X, Y) integers, x = X * 2^-s for one s common to the cloud; None for a point with a non-finite coordinate"""
    pts = np.asarray(points, F32).reshape(-1, 2)
    ratios = [[float(v).as_integer_ratio() if math.isfinite(v) else None for v in row] for row in pts.tolist()]
    s = max([r[1].bit_length() - 1 for row in ratios for r in row if r is not None] or [0])
    out = []
    for row in ratios:
        if row[0] is None or row[1] is None:
            out.append(None)
        else:
            out.append(tuple(r[0] << (s - (r[1].bit_length() - 1)) for r in row))
    return out


def sign(v):
    return (v > 0) - (v < 0)


def orient(a, b, c):
    """> 0: a, b, c turn counter-clockwise"""
    return (a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0])


def nearer(o, a, b):
    """|a - o|^2 - |b - o|^2: negative when a is nearer to o than b"""
    return (a[0] - o[0]) ** 2 + (a[1] - o[1]) ** 2 - (b[0] - o[0]) ** 2 - (b[1] - o[1]) ** 2


def incircle_det(a, b, c, d):
    """| x y x^2+y^2 1 | over a, b, c, d: positive when d is strictly inside the circle through the counter-clockwise a, b, c"""
    ax, ay, bx, by, cx, cy = a[0] - d[0], a[1] - d[1], b[0] - d[0], b[1] - d[1], c[0] - d[0], c[1] - d[1]
    return ((ax * ax + ay * ay) * (bx * cy - cx * by) + (bx * bx + by * by) * (cx * ay - ax * cy) + (cx * cx + cy * cy) * (ax * by - bx * ay))


def incircle_sos(P, ia, ib, ic, id_):
    """the sign of the in-circle determinant of points ia, ib, ic, id_ of P, with the lifted height of point p raised by eps_p,
    eps_0 >> eps_1 >> ...: at a zero determinant, the first non-zero cofactor in ascending point index"""
    a, b, c, d = P[ia], P[ib], P[ic], P[id_]
    s = sign(incircle_det(a, b, c, d))
    if s:
        return s
    cof = {ia: orient(b, c, d), ib: -orient(a, c, d), ic: orient(a, b, d), id_: -orient(a, b, c)}
    for p in sorted(cof):
        if cof[p]:
            return sign(cof[p])
    return 0


def usable(points):
    """(P, mask): the integer points, and which take part -- finite, and no lower-indexed point has the same coordinates"""
    P = to_ints(points)
    seen, mask = set(), []
    for p in P:
        mask.append(p is not None and p not in seen)
        if p is not None:
            seen.add(p)
    return P, mask


def canonical(faces, P=None):
    """faces as rows (i, a, b) with the lowest index first -- counter-clockwise when the integer points P are given -- sorted"""
    out = []
    for f in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        k = f.index(min(f))
        f = f[k:] + f[:k]
        if P is not None and orient(P[f[0]], P[f[1]], P[f[2]]) < 0:
            f = [f[0], f[2], f[1]]
        out.append(tuple(f))
    return sorted(out)


# ------------------------------------------------------------------------------------------------------------------------------ (b) check
def check(points, faces):
    """Asserts that `faces` ([M,3], any rotation) is the triangulation the header defines for `points` and returns the number of exact
    ties (interior edges whose four points are cocircular)."""
    P, ok = usable(points)
    live = [i for i, m in enumerate(ok) if m]
    n = len(live)
    faces = [tuple(int(v) for v in f) for f in np.asarray(faces, np.int64).reshape(-1, 3)]
    apex = {}
    for f in faces:
        assert all(0 <= v < len(P) and ok[v] for v in f), f"face {f} names a skipped point"
        assert orient(P[f[0]], P[f[1]], P[f[2]]) > 0, f"face {f} is not strictly counter-clockwise"
        for q in range(3):
            e = (f[q], f[(q + 1) % 3])
            assert e not in apex, f"directed edge {e} appears twice"
            apex[e] = f[(q + 2) % 3]
    ties = hull = 0
    for (a, b), c in apex.items():
        if (b, a) in apex:
            if a < b:
                det = incircle_det(P[a], P[b], P[c], P[apex[(b, a)]])
                assert det <= 0, f"edge {(a, b)} is not locally Delaunay"
                ties += det == 0
        else:
            hull += 1
            for p in live:
                o = orient(P[a], P[b], P[p])
                assert o >= 0, f"point {p} is right of the boundary edge {(a, b)}"
                if o == 0 and p not in (a, b):
                    t = (P[p][0] - P[a][0]) * (P[b][0] - P[a][0]) + (P[p][1] - P[a][1]) * (P[b][1] - P[a][1])
                    assert not 0 < t < (P[b][0] - P[a][0]) ** 2 + (P[b][1] - P[a][1]) ** 2, f"point {p} lies inside the boundary edge {(a, b)}"
    collinear = n < 3 or all(orient(P[live[0]], P[live[1]], P[p]) == 0 for p in live[2:])
    if collinear:
        assert not faces, "collinear points have no faces"
    else:
        assert {v for f in faces for v in f} == set(live), "a usable point is in no face"
        assert len(faces) == 2 * n - 2 - hull, f"M = {len(faces)}, 2n - 2 - h = {2 * n - 2 - hull}"
    return int(ties)


# ------------------------------------------------------------------------------------------------------------------------------- (c) walk
def _apex(P, live, u, v):
    """among the usable points strictly left of u -> v the one that no other beats; None when there is none"""
    best = None
    for k in live:
        if k == u or k == v or orient(P[u], P[v], P[k]) <= 0:
            continue
        if best is None or incircle_sos(P, u, v, best, k) > 0:
            best = k
    return best


def walk(points):
    """the faces of the library, in its order: rows (i, a, b), i the lowest index, counter-clockwise, sorted"""
    P, ok = usable(points)
    live = [i for i, m in enumerate(ok) if m]
    faces = []
    for i in live:
        j0 = None
        for k in live:
            if k != i and (j0 is None or nearer(P[i], P[k], P[j0]) < 0):
                j0 = k
        if j0 is None:
            continue
        j, closed, steps = j0, False, 0
        while True:
            k = _apex(P, live, i, j)
            if k is None:
                break
            steps += 1
            assert steps <= len(P), "the walk does not end"
            if i < j and i < k:
                faces.append((i, j, k))
            if k == j0:
                closed = True
                break
            j = k
        j = j0
        while not closed:
            k = _apex(P, live, j, i)
            if k is None:
                break
            steps += 1
            assert steps <= len(P), "the walk does not end"
            if i < j and i < k:
                faces.append((i, k, j))
            j = k
    return sorted(faces)


def edges_of(faces):
    """the undirected edges of a face list, (i, j) with i < j, sorted"""
    return sorted({(min(f[q], f[(q + 1) % 3]), max(f[q], f[(q + 1) % 3])) for f in faces for q in range(3)})


# --------------------------------------------------------------------------------------------------------------------- (d) threshold loop
def threshold_loop(points2d, faces, norm_threshold):
    """the reference's loop: every simplex's three edges; an edge longer than norm_threshold is not collected and spoils its face.
    float64 lengths.  -> (sorted edges, kept faces in the order given)"""
    pts = np.asarray(points2d, np.float64)
    edges, kept = set(), []
    for simplex in faces:
        valid = True
        for q in range(3):
            p1, p2 = int(simplex[q]), int(simplex[(q + 1) % 3])
            norm = float(np.linalg.norm(pts[p1] - pts[p2]))
            if norm_threshold is not None and norm > norm_threshold:
                valid = False
            else:
                edges.add((min(p1, p2), max(p1, p2)))
        if valid:
            kept.append(tuple(int(v) for v in simplex))
    return sorted(edges), kept


def gap_threshold(points2d, faces, quantile=0.6, rel=1e-4):
    """a threshold from the middle of a gap of at least `rel` (relative) in the sorted float64 edge lengths, at or above the given
    quantile: float32 and float64 lengths then fall on the same side of it"""
    pts = np.asarray(points2d, np.float64)
    lens = np.sort([np.linalg.norm(pts[a] - pts[b]) for a, b in edges_of(faces)])
    for q in range(int(len(lens) * quantile), len(lens) - 1):
        if lens[q + 1] - lens[q] >= rel * lens[q + 1]:
            return float(0.5 * (lens[q] + lens[q + 1]))
    raise AssertionError("no gap in the edge lengths")


# ----------------------------------------------------------------------------------------------------------------------------- the clouds
CIRCLE65 = sorted({(sx * x, sy * y) for a, b in ((65, 0), (16, 63), (25, 60), (33, 56), (39, 52)) for x, y in ((a, b), (b, a))
                   for sx in (1, -1) for sy in (1, -1)})
assert len(CIRCLE65) == 36 and all(x * x + y * y == 4225 for x, y in CIRCLE65)


def grid(n, spacing=1.0):
    """n x n points (i, j) * spacing, the product formed in float32"""
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2).astype(F32)
    return (ij * F32(spacing)).astype(F32)


def degenerate_clouds():
    """name -> (float32 [N,2], number of skipped points)"""
    rng = np.random.default_rng(5)
    circle = np.array(CIRCLE65, F32)
    inner = np.array([(0, 0), (10, 5), (-20, 7), (3, -40), (30, 30), (-1, 1), (12, -12)], F32)
    dup = rng.random((40, 2)).astype(F32)
    dup[[7, 19, 33]] = dup[[2, 2, 11]]
    dup[25, 1] = np.nan
    dup[3] = (0.0, 0.25)
    dup[30] = (-0.0, 0.25)                                                   # -0.0 == 0.0: a fourth duplicate
    mags = np.array([1e-45, 1e-38, 1e-20, 1e-3, 1.0, 1e5, 1e12, 1e30])
    mixed = (rng.choice(mags, (24, 2)) * rng.choice([-1.0, 1.0], (24, 2)) * rng.integers(1, 9, (24, 2))).astype(F32)
    hull = np.array([(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 2), (4, 4), (2, 4), (0, 4), (0, 3), (0, 1), (1, 1), (3, 2), (2, 2)], F32)
    return {
        "square": (np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F32), 0),
        "collinear4": (np.array([(0, 0), (1, 1), (3, 3), (2, 2)], F32), 0),
        "hull_collinear": (hull, 0),
        "grid9": (grid(9), 0),
        "grid17": (grid(17), 0),
        "grid9_permuted": (grid(9)[rng.permutation(81)], 0),
        "grid8_small": (grid(8, 0.00625), 0),
        "circle65": (circle, 0),
        "circle65_inner": (np.concatenate([inner, circle]), 0),
        "circle65_centre": (np.concatenate([inner[:1], circle]), 0),            # point 0 has all 36 others as neighbours
        "duplicates_nan": (dup, 5),
        # the float32 range: every coordinate a denormal; near the top of the range; and magnitudes 60 binades apart in one cloud
        "circle65_denormal": ((circle.astype(np.float64) * 2.0 ** -140).astype(F32), 0),
        "grid8_huge": ((grid(8).astype(np.float64) * 2.0 ** 120).astype(F32), 0),
        "mixed_magnitudes": (mixed, 0),
    }


def size_clouds():
    """seeded uniform clouds at the sizes around a wave's 64 lanes, and the empty ones"""
    rng = np.random.default_rng(21)
    return {f"n{n}": rng.random((n, 2)).astype(F32) for n in (0, 1, 2, 3, 63, 64, 65, 96)}


# ---------------------------------------------------------------------------------------------------------------------------- the fixture
def fixture_cloud(n, seed):
    return np.random.default_rng(seed).random((n, 2), dtype=F32)


def scipy_faces(points):
    """SciPy's triangulation of the float32 cloud as canonical rows"""
    from scipy.spatial import Delaunay
    return np.array(canonical(Delaunay(np.asarray(points, np.float64)).simplices, to_ints(points)), np.int32)


def make_fixture(path=GOLDEN):
    out = {}
    for n, seed in FIXTURE_CLOUDS:
        pts = fixture_cloud(n, seed)
        out[f"points_{n}"], out[f"faces_{n}"] = pts, scipy_faces(pts)
    np.savez_compressed(path, **out)


def load_fixture():
    z = np.load(GOLDEN)
    return {n: (z[f"points_{n}"], z[f"faces_{n}"]) for n, _seed in FIXTURE_CLOUDS}


# ------------------------------------------------------------------------------------------------------- (e) adversarial predicate inputs
ORIENT, NEARER, INCIRCLE = 0, 1, 2
RECORD_WORDS = 13        # kind, four indices, four points


def _ulp(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


def adversarial_records(seed=3):
    """list of (kind, idx [4], xy float32 [4,2]): exactly cocircular integer sets scaled by powers of two, the same with one coordinate
    one ulp off, collinear triples +- one ulp, magnitudes mixed from denormals to 1e30, random values"""
    rng = np.random.default_rng(seed)
    circle = np.array(CIRCLE65, np.float64)
    rec = []

    def add(kind, xy, idx=None):
        xy = np.asarray(xy, F32).reshape(4, 2)
        assert np.isfinite(xy).all()
        rec.append((kind, [int(v) for v in (rng.permutation(1000)[:4] if idx is None else idx)], xy))

    def nudged(xy):
        """the points, then each with one coordinate one ulp up or down"""
        yield xy
        for _ in range(3):
            q = np.array(xy, F32)
            r, c = rng.integers(q.shape[0]), rng.integers(2)
            q[r, c] = _ulp(q[r, c], rng.integers(2))
            yield q

    for scale in (2.0 ** -149, 2.0 ** -140, 2.0 ** -126, 2.0 ** -60, 2.0 ** -7, 1.0, 2.0 ** 40, 2.0 ** 100, 2.0 ** 121):
        for _ in range(12):
            four = (circle[rng.choice(36, 4, replace=False)] * scale).astype(F32)
            for q in nudged(four):
                add(INCIRCLE, q)
                add(INCIRCLE, q, idx=sorted(rng.permutation(50)[:4].tolist()))
            # two points at equal distance from the centre (0, 0)
            three = np.concatenate([np.zeros((1, 2)), circle[rng.choice(36, 2, replace=False)] * scale]).astype(F32)
            for q in nudged(three):
                add(NEARER, np.concatenate([q, q[:1]]))
            # collinear triples: k * (dx, dy) from a base point, all exact in float32
            base, step = rng.integers(-50, 50, 2), rng.integers(-9, 10, 2)
            tri = (np.array([base + k * step for k in rng.choice(12, 3, replace=False)], np.float64) * scale).astype(F32)
            for q in nudged(tri):
                add(ORIENT, np.concatenate([q, q[:1]]))
            # three collinear and a fourth: the in-circle determinant loses a cofactor
            add(INCIRCLE, np.concatenate([tri, four[:1]]))
            add(INCIRCLE, np.concatenate([four[:1], tri]))
    # a regular grid's unit squares and the 0.00625f grid's
    for g in (grid(4), grid(4, 0.00625)):
        for _ in range(40):
            i, j = rng.integers(0, 3, 2)
            quad = g.reshape(4, 4, 2)[[i, i + 1, i + 1, i], [j, j, j + 1, j + 1]]
            add(INCIRCLE, quad[rng.permutation(4)])
    # magnitudes mixed over the whole range, denormals too; and plain random values
    mags = np.array([1e-45, 3e-42, 1e-38, 1.1754944e-38, 1e-30, 1e-12, 1e-3, 1.0, 7.0, 1e5, 1e12, 1e21, 1e30], np.float64)
    for _ in range(400):
        xy = (rng.choice(mags, (4, 2)) * rng.choice([-1.0, 1.0], (4, 2)) * rng.integers(1, 9, (4, 2))).astype(F32)
        for kind in (ORIENT, NEARER, INCIRCLE):
            add(kind, xy)
    for _ in range(400):
        xy = rng.standard_normal((4, 2)).astype(F32)
        if rng.integers(2):
            xy[3] = xy[rng.integers(3)]                                      # a repeated point
        for kind in (ORIENT, NEARER, INCIRCLE):
            add(kind, xy)
    return rec


def pack_records(rec):
    """the file the host program reads: int32 count, then RECORD_WORDS 32-bit words per record (the coordinates as their bits)"""
    words = np.zeros((len(rec), RECORD_WORDS), np.int32)
    for r, (kind, idx, xy) in enumerate(rec):
        words[r, 0], words[r, 1:5], words[r, 5:] = kind, idx, np.asarray(xy, F32).reshape(8).view(np.int32)
    return np.int32(len(rec)).tobytes() + words.tobytes()


def expected_signs(rec):
    out = []
    for kind, idx, xy in rec:
        P = to_ints(xy)
        if kind == ORIENT:
            out.append(sign(orient(P[0], P[1], P[2])))
        elif kind == NEARER:
            out.append(sign(nearer(P[0], P[1], P[2])))
        else:
            out.append(incircle_sos(dict(zip(idx, P)), *idx))
    return out
