// csplat_zbuffer.hip -- the mesh z-buffer: depth, silhouette and face-id images of a triangle mesh, and of a point cloud as one-pixel
// primitives (gfx950, wave64; include/csplat.h, csplat_zb_mesh, csplat_zb_points and csplat_zb_mark, states the semantics).  The reference
// answers "what would a depth camera see of this mesh" on the host: Blender renders (manipulation/fold_rendering/) and the Python double
// loop build_depth_from_pointcloud (manipulation/envs/camera_utils.py:7-41).
//   k_zb_project   one thread per (view, vertex): p_cam, the pixel, the snapped coordinates, 1 / z and the validity -> one 16-byte record
//   k_zb_clear     the per-pixel keys to all-ones, 16 bytes a lane; every call does it
//   k_zb_draw      one workgroup of four waves per (view, face): the waves stride over the 8 x 8-pixel blocks of the face's bounding box
//                  clipped to the image, a lane per pixel (a row of a block is 8 contiguous pixels); a block that lies wholly outside one
//                  edge (the edge function negative at its four corner pixels) is skipped; coverage in exact int64 arithmetic; a covered
//                  pixel offers the key (float bits of z) << 32 | face with one 64-bit integer atomicMin
//   k_zb_points    one thread per (view, point): the same projection, the pixel (rint(px), rint(py)), the same key with the point index
//   k_zb_resolve   one thread per pixel: the winner's key -> depth (the key's own z, or z along the pixel's ray), silhouette, id and, for
//                  a mesh, the perspective-correct weights recomputed with the operations of the draw; plain stores
//   k_zb_mark      one thread per pixel with face_id >= 0: byte 1 into face_visible and into node_visible of the three corners
// The only atomic is the unsigned 64-bit integer minimum, which does not depend on the order of arrival: every output is bit-reproducible.
// No float atomics.  Float arithmetic without contraction: every operation is one float32 rounding, divisions and the square root the
// correctly rounded ones, so that a numpy float32 restatement gives the same bits.
// Algorithmic bytes: project 12 read and 16 written per (view, vertex); clear 8 written per pixel; draw 12 + 48 read per (view, face) and
// one 8-byte atomic request per covered (face, pixel) pair; resolve 8 read and 12 written per pixel (+ 12 with the weights).
#include "csplat_common.h"
#include "csplat_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int ZB_THREADS = 256;
constexpr int ZB_SUB = 256;                    // snapped units per pixel
constexpr float ZB_GUARD = 16384.f;            // |px|, |py| of a valid vertex: 256 * 16384 = 2^22, so every edge function fits int64 with room
constexpr int ZB_BLOCK = 8;                    // a wave's block of pixels is ZB_BLOCK x ZB_BLOCK
constexpr unsigned long long ZB_EMPTY = ~0ull;

struct ZbProjected { float px, py, z, iz; bool valid; };

// stage P.  intr = (fx, fy, cx, cy), w2c = 3 x 4 row-major world-to-camera, both wave-uniform
__device__ __forceinline__ ZbProjected zb_project(const float *__restrict__ p, const float *__restrict__ intr, const float *__restrict__ w2c, float near) {
    const float X = p[0], Y = p[1], Z = p[2];
    const float x = w2c[0] * X + w2c[1] * Y + w2c[2] * Z + w2c[3];
    const float y = w2c[4] * X + w2c[5] * Y + w2c[6] * Z + w2c[7];
    ZbProjected r;
    r.z = w2c[8] * X + w2c[9] * Y + w2c[10] * Z + w2c[11];
    r.px = __fdiv_rn(intr[0] * x, r.z) + intr[2];
    r.py = __fdiv_rn(intr[1] * y, r.z) + intr[3];
    r.iz = __fdiv_rn(1.f, r.z);
    r.valid = finite_f32(x) && finite_f32(y) && finite_f32(r.z) && finite_f32(r.px) && finite_f32(r.py) && finite_f32(r.iz) && r.z > near &&
              fabsf(r.px) <= ZB_GUARD && fabsf(r.py) <= ZB_GUARD;
    return r;
}

// grid (vertices, V views); vstride = 0 (one mesh for all views) or 3 N
__global__ __launch_bounds__(ZB_THREADS) void k_zb_project(int64_t N, const float *__restrict__ vertices, int64_t vstride,
                                                           const float *__restrict__ intrinsics, const float *__restrict__ world_to_cam, float near,
                                                           int4 *__restrict__ screen) {
    const int64_t n = (int64_t)blockIdx.x * ZB_THREADS + threadIdx.x;
    if (n >= N) return;
    const int v = blockIdx.y;
    const ZbProjected r = zb_project(vertices + (int64_t)v * vstride + 3 * n, intrinsics + 4 * v, world_to_cam + 12 * v, near);
    int4 rec = make_int4(0, 0, 0, 0);
    if (r.valid) rec = make_int4((int)rintf((float)ZB_SUB * r.px), (int)rintf((float)ZB_SUB * r.py), __float_as_int(r.iz), 1);
    screen[(int64_t)v * N + n] = rec;
}

__global__ __launch_bounds__(ZB_THREADS) void k_zb_clear(int64_t n16, uint4 *__restrict__ keys16) {
    const int64_t i = (int64_t)blockIdx.x * ZB_THREADS + threadIdx.x;
    if (i < n16) keys16[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// a face after stage D's set-up: the working corners (1 and 2 swapped when the snapped area is negative), A > 0; iz in the face's own order
struct ZbFace {
    int64_t x0, y0, x1, y1, x2, y2, A;
    float iz[3];
    bool swapped;
};

// false: the face is dropped (a corner index outside [0, N), an invalid corner, no area)
__device__ __forceinline__ bool zb_face(const int32_t *__restrict__ faces, int64_t f, int64_t N, const int4 *__restrict__ sv, ZbFace &t) {
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= N || i1 < 0 || i1 >= N || i2 < 0 || i2 >= N) return false;
    const int4 a = sv[i0];
    int4 b = sv[i1], c = sv[i2];
    if (!(a.w && b.w && c.w)) return false;
    t.iz[0] = __int_as_float(a.z); t.iz[1] = __int_as_float(b.z); t.iz[2] = __int_as_float(c.z);
    t.A = (int64_t)(b.x - a.x) * (c.y - a.y) - (int64_t)(b.y - a.y) * (c.x - a.x);
    if (t.A == 0) return false;
    t.swapped = t.A < 0;
    if (t.swapped) { const int4 h = b; b = c; c = h; t.A = -t.A; }
    t.x0 = a.x; t.y0 = a.y; t.x1 = b.x; t.y1 = b.y; t.x2 = c.x; t.y2 = c.y;
    return true;
}

// the edge function of a -> b at the snapped point (px, py)
__device__ __forceinline__ int64_t zb_edge(int64_t xa, int64_t ya, int64_t xb, int64_t yb, int64_t px, int64_t py) {
    return (xb - xa) * (py - ya) - (yb - ya) * (px - xa);
}
// the top-left rule: inside, or on an edge that the face owns
__device__ __forceinline__ bool zb_owns(int64_t E, int64_t dx, int64_t dy) { return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0))); }

// E01, E12, E20 of the working corners -> the weights b of the face's own corners, q and z
__device__ __forceinline__ float zb_depth(const ZbFace &t, int64_t E01, int64_t E12, int64_t E20, float b[3], float &q) {
    const float fA = (float)t.A;
    const float w0 = __fdiv_rn((float)E12, fA), w1 = __fdiv_rn((float)E20, fA), w2 = __fdiv_rn((float)E01, fA);
    b[0] = w0;
    b[1] = t.swapped ? w2 : w1;
    b[2] = t.swapped ? w1 : w2;
    q = b[0] * t.iz[0] + b[1] * t.iz[1] + b[2] * t.iz[2];
    return __fdiv_rn(1.f, q);
}

__device__ __forceinline__ int64_t zb_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
__device__ __forceinline__ int64_t zb_min3(int64_t a, int64_t b, int64_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
__device__ __forceinline__ int64_t zb_max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// grid (F faces, V views).  Everything up to the lane's own pixel is uniform over the workgroup
__global__ __launch_bounds__(ZB_THREADS) void k_zb_draw(int64_t N, int H, int W, const int32_t *__restrict__ faces, const int4 *__restrict__ screen,
                                                        unsigned long long *__restrict__ keys) {
    const int64_t f = blockIdx.x;
    const int v = blockIdx.y;
    ZbFace t;
    if (!zb_face(faces, f, N, screen + (int64_t)v * N, t)) return;
    // the pixels whose centres lie in the bounding box: 256 X >= min and 256 X <= max, clipped to the image
    int64_t X0 = -zb_floor_div(-zb_min3(t.x0, t.x1, t.x2), ZB_SUB), X1 = zb_floor_div(zb_max3(t.x0, t.x1, t.x2), ZB_SUB);
    int64_t Y0 = -zb_floor_div(-zb_min3(t.y0, t.y1, t.y2), ZB_SUB), Y1 = zb_floor_div(zb_max3(t.y0, t.y1, t.y2), ZB_SUB);
    X0 = X0 < 0 ? 0 : X0; Y0 = Y0 < 0 ? 0 : Y0;
    X1 = X1 > W - 1 ? W - 1 : X1; Y1 = Y1 > H - 1 ? H - 1 : Y1;
    if (X0 > X1 || Y0 > Y1) return;
    const int bx0 = (int)(X0 / ZB_BLOCK), by0 = (int)(Y0 / ZB_BLOCK);
    const int nbx = (int)(X1 / ZB_BLOCK) - bx0 + 1, nby = (int)(Y1 / ZB_BLOCK) - by0 + 1;
    const int64_t n_blocks = (int64_t)nbx * nby;
    const int64_t dx01 = t.x1 - t.x0, dy01 = t.y1 - t.y0, dx12 = t.x2 - t.x1, dy12 = t.y2 - t.y1, dx20 = t.x0 - t.x2, dy20 = t.y0 - t.y2;
    const int lane = threadIdx.x & 63, lx = lane & (ZB_BLOCK - 1), ly = lane >> 3;
    const int64_t far = (int64_t)ZB_SUB * (ZB_BLOCK - 1);
    for (int64_t blk = threadIdx.x >> 6; blk < n_blocks; blk += ZB_THREADS / 64) {
        const int bx = bx0 + (int)(blk % nbx), by = by0 + (int)(blk / nbx);
        const int64_t px = (int64_t)ZB_SUB * ZB_BLOCK * bx, py = (int64_t)ZB_SUB * ZB_BLOCK * by;
        const int64_t E01 = zb_edge(t.x0, t.y0, t.x1, t.y1, px, py), E12 = zb_edge(t.x1, t.y1, t.x2, t.y2, px, py),
                      E20 = zb_edge(t.x2, t.y2, t.x0, t.y0, px, py);
        // an edge function is affine: negative at the four corner pixels of the block = negative at every pixel of it
        const bool out01 = E01 < 0 && E01 - dy01 * far < 0 && E01 + dx01 * far < 0 && E01 + dx01 * far - dy01 * far < 0;
        const bool out12 = E12 < 0 && E12 - dy12 * far < 0 && E12 + dx12 * far < 0 && E12 + dx12 * far - dy12 * far < 0;
        const bool out20 = E20 < 0 && E20 - dy20 * far < 0 && E20 + dx20 * far < 0 && E20 + dx20 * far - dy20 * far < 0;
        if (out01 || out12 || out20) continue;
        const int X = bx * ZB_BLOCK + lx, Y = by * ZB_BLOCK + ly;
        if (X < X0 || X > X1 || Y < Y0 || Y > Y1) continue;                                   // (inside the image: the box is clipped to it)
        const int64_t sx = (int64_t)ZB_SUB * lx, sy = (int64_t)ZB_SUB * ly;
        const int64_t e01 = E01 + dx01 * sy - dy01 * sx, e12 = E12 + dx12 * sy - dy12 * sx, e20 = E20 + dx20 * sy - dy20 * sx;
        if (!(zb_owns(e01, dx01, dy01) && zb_owns(e12, dx12, dy12) && zb_owns(e20, dx20, dy20))) continue;
        float b[3], q;
        const float z = zb_depth(t, e01, e12, e20, b, q);
        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(uint32_t)f;
        atomicMin(keys + ((int64_t)v * H + Y) * W + X, key);
    }
}

// grid (points, V views)
__global__ __launch_bounds__(ZB_THREADS) void k_zb_points(int64_t M, int H, int W, const float *__restrict__ points, int64_t pstride,
                                                          const float *__restrict__ intrinsics, const float *__restrict__ world_to_cam, float near,
                                                          unsigned long long *__restrict__ keys) {
    const int64_t m = (int64_t)blockIdx.x * ZB_THREADS + threadIdx.x;
    if (m >= M) return;
    const int v = blockIdx.y;
    const ZbProjected r = zb_project(points + (int64_t)v * pstride + 3 * m, intrinsics + 4 * v, world_to_cam + 12 * v, near);
    if (!r.valid) return;
    const float fx = rintf(r.px), fy = rintf(r.py);                                            // (|px| <= 16384: exact integers)
    if (!(fx >= 0.f && fx <= (float)(W - 1) && fy >= 0.f && fy <= (float)(H - 1))) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(r.z) << 32) | (unsigned long long)(uint32_t)m;
    atomicMin(keys + ((int64_t)v * H + (int)fy) * W + (int)fx, key);
}

// one thread per pixel of all views.  MESH: silhouette and (bary != NULL) the weights; otherwise depth and id only
template <bool MESH>
__global__ __launch_bounds__(ZB_THREADS) void k_zb_resolve(int64_t total, int H, int W, int64_t N, const unsigned long long *__restrict__ keys,
                                                           const float *__restrict__ intrinsics, int kind, const int32_t *__restrict__ faces,
                                                           const int4 *__restrict__ screen, float *__restrict__ depth,
                                                           float *__restrict__ silhouette, int32_t *__restrict__ id, float *__restrict__ bary) {
    const int64_t p = (int64_t)blockIdx.x * ZB_THREADS + threadIdx.x;
    if (p >= total) return;
    const int64_t HW = (int64_t)H * W;
    const int v = (int)(p / HW);
    const int64_t pix = p - (int64_t)v * HW;
    const int Y = (int)(pix / W), X = (int)(pix - (int64_t)Y * W);
    const unsigned long long key = keys[p];
    const bool hit = key != ZB_EMPTY;
    const float z = __uint_as_float((uint32_t)(key >> 32));
    float d = 0.f;
    if (hit) {
        d = z;
        if (kind == 1) {
            const float *__restrict__ k = intrinsics + 4 * v;
            const float u = __fdiv_rn((float)X - k[2], k[0]), w = __fdiv_rn((float)Y - k[3], k[1]);
            d = z * __fsqrt_rn(u * u + w * w + 1.f);
        }
    }
    depth[p] = d;
    id[p] = hit ? (int32_t)(uint32_t)key : -1;
    if (!MESH) return;
    silhouette[p] = hit ? 1.f : 0.f;
    if (!bary) return;
    float t3[3] = {0.f, 0.f, 0.f};
    ZbFace t;
    if (hit && zb_face(faces, (int64_t)(uint32_t)key, N, screen + (int64_t)v * N, t)) {
        const int64_t px = (int64_t)ZB_SUB * X, py = (int64_t)ZB_SUB * Y;
        float b[3], q;
        zb_depth(t, zb_edge(t.x0, t.y0, t.x1, t.y1, px, py), zb_edge(t.x1, t.y1, t.x2, t.y2, px, py), zb_edge(t.x2, t.y2, t.x0, t.y0, px, py), b, q);
#pragma unroll
        for (int i = 0; i < 3; i++) t3[i] = __fdiv_rn(b[i] * t.iz[i], q);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) bary[((int64_t)v * 3 + i) * HW + pix] = t3[i];
}

// every writer stores the value 1 into flags zeroed on the stream before the launch
__global__ __launch_bounds__(ZB_THREADS) void k_zb_mark(int64_t total, int64_t HW, int64_t N, int64_t F, const int32_t *__restrict__ face_id,
                                                        const int32_t *__restrict__ faces, uint8_t *__restrict__ face_visible,
                                                        uint8_t *__restrict__ node_visible) {
    const int64_t p = (int64_t)blockIdx.x * ZB_THREADS + threadIdx.x;
    if (p >= total) return;
    const int64_t f = face_id[p];
    if (f < 0 || f >= F) return;
    const int64_t v = p / HW;
    face_visible[v * F + f] = 1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int64_t n = faces[3 * f + c];
        if (n >= 0 && n < N) node_visible[v * N + n] = 1;
    }
}

struct ZbRange { const void *p; size_t n; };

// no output may share a byte with another operand; inputs may share among themselves.  `n_out` leading ranges are the outputs
bool zb_any_overlap(const ZbRange *r, int n, int n_out) {
    for (int i = 0; i < n_out; i++)
        for (int j = i + 1; j < n; j++) {
            if (!r[i].p || !r[j].p || r[i].n == 0 || r[j].n == 0) continue;
            const uintptr_t x = (uintptr_t)r[i].p, y = (uintptr_t)r[j].p;
            if (x < y + r[j].n && y < x + r[i].n) return true;
        }
    return false;
}

struct ZbCarve { size_t keys, screen, total; };
ZbCarve zb_carve(int64_t pixels, int64_t records) {
    ZbCarve c;
    c.keys = 0;
    c.screen = align256((size_t)pixels * 8);          // (a multiple of 16: k_zb_clear may write one key beyond an odd count)
    c.total = c.screen + align256((size_t)records * 16);
    return c;
}

constexpr int64_t ZB_2_31 = (int64_t)1 << 31;

bool zb_sizes_ok(int V, int64_t n, int H, int W) {
    return V >= 0 && V <= 65535 && n >= 0 && n < ZB_2_31 && H >= 0 && W >= 0 && (int64_t)H * W < ZB_2_31 && (int64_t)V * H * W < ZB_2_31 &&
           (int64_t)V * n < ZB_2_31;
}

int zb_clear(hipStream_t s, int64_t pixels, void *keys) {
    const int64_t n16 = (pixels + 1) / 2;
    k_zb_clear<<<(unsigned)cdiv(n16, ZB_THREADS), ZB_THREADS, 0, s>>>(n16, (uint4 *)keys);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int csplat_zb_mesh(void *stream, int V, int64_t N, int64_t F, int H, int W, const float *vertices, int per_view, const int32_t *faces,
                              const float *intrinsics, const float *world_to_cam, float near, int kind, float *depth, float *silhouette,
                              int32_t *face_id, float *bary, int32_t *screen, void *temp, size_t temp_bytes) {
    CSPLAT_REQUIRE(zb_sizes_ok(V, N, H, W), "csplat_zb_mesh: 0 <= V <= 65535, 0 <= N < 2^31, H and W >= 0, V * H * W < 2^31, V * N < 2^31");
    CSPLAT_REQUIRE(F >= 0 && F < ZB_2_31, "csplat_zb_mesh: 0 <= F < 2^31");
    CSPLAT_REQUIRE(kind == 0 || kind == 1, "csplat_zb_mesh: kind is 0 (view-space z) or 1 (distance along the ray)");
    CSPLAT_REQUIRE(near >= 0.f && near < __builtin_inff(), "csplat_zb_mesh: near is a finite number >= 0");
    CSPLAT_REQUIRE(per_view == 0 || per_view == 1, "csplat_zb_mesh: per_view is 0 (vertices [N][3]) or 1 ([V][N][3])");
    const int64_t pixels = (int64_t)V * H * W, records = (int64_t)V * N;
    if (pixels == 0 && (records == 0 || !screen)) return 0;
    CSPLAT_REQUIRE(intrinsics && world_to_cam && temp, "csplat_zb_mesh: a NULL operand");
    CSPLAT_REQUIRE(records == 0 || vertices, "csplat_zb_mesh: NULL vertices with N > 0");
    CSPLAT_REQUIRE(F == 0 || faces, "csplat_zb_mesh: NULL faces with F > 0");
    CSPLAT_REQUIRE(pixels == 0 || (depth && silhouette && face_id), "csplat_zb_mesh: a NULL output");
    CSPLAT_REQUIRE((((uintptr_t)vertices | (uintptr_t)faces | (uintptr_t)intrinsics | (uintptr_t)world_to_cam | (uintptr_t)depth |
                     (uintptr_t)silhouette | (uintptr_t)face_id | (uintptr_t)bary) & 3u) == 0 && (((uintptr_t)screen | (uintptr_t)temp) & 15u) == 0,
                   "csplat_zb_mesh: operands must be 4-byte aligned, screen and temp 16-byte aligned");
    const ZbCarve c = zb_carve(pixels, records);
    CSPLAT_REQUIRE(temp_bytes >= c.total, "csplat_zb_mesh: temp_bytes is below align256(8 V H W) + align256(16 V N)");
    const ZbRange r[] = {{depth, (size_t)pixels * 4}, {silhouette, (size_t)pixels * 4}, {face_id, (size_t)pixels * 4}, {bary, (size_t)pixels * 12},
                         {screen, (size_t)records * 16}, {temp, c.total}, {vertices, (size_t)(per_view ? records : N) * 12}, {faces, (size_t)F * 12},
                         {intrinsics, (size_t)V * 16}, {world_to_cam, (size_t)V * 48}};
    CSPLAT_REQUIRE(!zb_any_overlap(r, 10, 6), "csplat_zb_mesh: an output or temp overlaps another operand");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *keys = (unsigned long long *)((char *)temp + c.keys);
    int4 *sv = screen ? (int4 *)screen : (int4 *)((char *)temp + c.screen);
    if (records > 0) {
        k_zb_project<<<dim3((unsigned)cdiv(N, ZB_THREADS), (unsigned)V), ZB_THREADS, 0, s>>>(N, vertices, per_view ? 3 * N : 0, intrinsics, world_to_cam,
                                                                                            near, sv);
        LAUNCH_CHECK();
    }
    if (pixels == 0) return 0;
    if (int rc = zb_clear(s, pixels, keys)) return rc;
    if (F > 0 && N > 0) {
        k_zb_draw<<<dim3((unsigned)F, (unsigned)V), ZB_THREADS, 0, s>>>(N, H, W, faces, sv, keys);
        LAUNCH_CHECK();
    }
    k_zb_resolve<true><<<(unsigned)cdiv(pixels, ZB_THREADS), ZB_THREADS, 0, s>>>(pixels, H, W, N, keys, intrinsics, kind, faces, sv, depth, silhouette,
                                                                                face_id, bary);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_zb_points(void *stream, int V, int64_t M, int H, int W, const float *points, int per_view, const float *intrinsics,
                                const float *world_to_cam, float near, int kind, float *depth, int32_t *point_id, void *temp, size_t temp_bytes) {
    CSPLAT_REQUIRE(zb_sizes_ok(V, M, H, W), "csplat_zb_points: 0 <= V <= 65535, 0 <= M < 2^31, H and W >= 0, V * H * W < 2^31, V * M < 2^31");
    CSPLAT_REQUIRE(kind == 0 || kind == 1, "csplat_zb_points: kind is 0 (view-space z) or 1 (distance along the ray)");
    CSPLAT_REQUIRE(near >= 0.f && near < __builtin_inff(), "csplat_zb_points: near is a finite number >= 0");
    CSPLAT_REQUIRE(per_view == 0 || per_view == 1, "csplat_zb_points: per_view is 0 (points [M][3]) or 1 ([V][M][3])");
    const int64_t pixels = (int64_t)V * H * W;
    if (pixels == 0) return 0;
    CSPLAT_REQUIRE(intrinsics && world_to_cam && temp && depth && point_id, "csplat_zb_points: a NULL operand");
    CSPLAT_REQUIRE(M == 0 || points, "csplat_zb_points: NULL points with M > 0");
    CSPLAT_REQUIRE((((uintptr_t)points | (uintptr_t)intrinsics | (uintptr_t)world_to_cam | (uintptr_t)depth | (uintptr_t)point_id) & 3u) == 0 &&
                       ((uintptr_t)temp & 15u) == 0, "csplat_zb_points: operands must be 4-byte aligned, temp 16-byte aligned");
    const ZbCarve c = zb_carve(pixels, (int64_t)V * M);
    CSPLAT_REQUIRE(temp_bytes >= c.total, "csplat_zb_points: temp_bytes is below align256(8 V H W) + align256(16 V M)");
    const ZbRange r[] = {{depth, (size_t)pixels * 4}, {point_id, (size_t)pixels * 4}, {temp, c.total}, {points, (size_t)(per_view ? V * M : M) * 12},
                         {intrinsics, (size_t)V * 16}, {world_to_cam, (size_t)V * 48}};
    CSPLAT_REQUIRE(!zb_any_overlap(r, 6, 3), "csplat_zb_points: an output or temp overlaps another operand");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *keys = (unsigned long long *)((char *)temp + c.keys);
    if (int rc = zb_clear(s, pixels, keys)) return rc;
    if (M > 0) {
        k_zb_points<<<dim3((unsigned)cdiv(M, ZB_THREADS), (unsigned)V), ZB_THREADS, 0, s>>>(M, H, W, points, per_view ? 3 * M : 0, intrinsics,
                                                                                           world_to_cam, near, keys);
        LAUNCH_CHECK();
    }
    k_zb_resolve<false><<<(unsigned)cdiv(pixels, ZB_THREADS), ZB_THREADS, 0, s>>>(pixels, H, W, M, keys, intrinsics, kind, nullptr, nullptr, depth,
                                                                                 nullptr, point_id, nullptr);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int csplat_zb_mark(void *stream, int V, int64_t N, int64_t F, int H, int W, const int32_t *face_id, const int32_t *faces,
                              uint8_t *face_visible, uint8_t *node_visible) {
    CSPLAT_REQUIRE(zb_sizes_ok(V, N, H, W), "csplat_zb_mark: 0 <= V <= 65535, 0 <= N < 2^31, H and W >= 0, V * H * W < 2^31, V * N < 2^31");
    CSPLAT_REQUIRE(F >= 0 && F < ZB_2_31 && (int64_t)V * F < ZB_2_31, "csplat_zb_mark: 0 <= F < 2^31, V * F < 2^31");
    const int64_t pixels = (int64_t)V * H * W, nf = (int64_t)V * F, nn = (int64_t)V * N;
    CSPLAT_REQUIRE((nf == 0 || face_visible) && (nn == 0 || node_visible), "csplat_zb_mark: NULL flags");
    CSPLAT_REQUIRE(pixels == 0 || F == 0 || (face_id && faces), "csplat_zb_mark: a NULL operand");
    CSPLAT_REQUIRE((((uintptr_t)face_id | (uintptr_t)faces) & 3u) == 0, "csplat_zb_mark: operands must be 4-byte aligned");
    const ZbRange r[] = {{face_visible, (size_t)nf}, {node_visible, (size_t)nn}, {face_id, (size_t)pixels * 4}, {faces, (size_t)F * 12}};
    CSPLAT_REQUIRE(!zb_any_overlap(r, 4, 2), "csplat_zb_mark: an output overlaps another operand");
    hipStream_t s = (hipStream_t)stream;
    if (nf > 0) HIP_TRY(hipMemsetAsync(face_visible, 0, (size_t)nf, s));
    if (nn > 0) HIP_TRY(hipMemsetAsync(node_visible, 0, (size_t)nn, s));
    if (pixels == 0 || F == 0) return 0;
    k_zb_mark<<<(unsigned)cdiv(pixels, ZB_THREADS), ZB_THREADS, 0, s>>>(pixels, (int64_t)H * W, N, F, face_id, faces, face_visible, node_visible);
    LAUNCH_CHECK();
    return 0;
}
