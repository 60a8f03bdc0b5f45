// csplat_camera_dataset.hip -- the camera data set on the device (gfx950, wave64; include/csplat.h "Camera data set" states the semantics).
// The reference's MDNerfDataset (scene_reconstruction/dataset.py:46-123) keeps float images on the host and builds a fresh Camera per item:
// every training step begins with host-to-device copies, or a torch.cat, of its three ground-truth images and masks.  Here the images live
// in ONE device buffer of slots -- as the 8-bit levels the loader quantised them to, or as float32 words -- and
//   k_camera_batch   ONE launch writes the step's gt [n][3][H][W] and mask [n][1][H][W].  The grid is (blocks of a plane, planes of a slot,
//                    cameras); a block covers CAMERA_THREADS * CAMERA_PIXELS_PER_LANE consecutive pixels of one plane.  A lane takes
//                    CAMERA_PIXELS_PER_LANE = 16 pixels as four groups of four, group j of lane l being group j * CAMERA_THREADS + l of
//                    the block: 16 bytes loaded (uint8 storage: four 4-byte words; float32 storage: four 16-byte loads), four 16-byte
//                    stores, and a wave's instruction reads 256 and writes 1024 CONSECUTIVE bytes.  (A lane that converted 16 consecutive
//                    pixels -- one 16-byte load, 64 consecutive bytes written by four instructions that each leave 48-byte holes between
//                    lanes -- took 13.6 us for 3 cameras of 800 x 800 with masks where this mapping takes 8.4 us, same MI355X, back-to-back
//                    launches between device events.)
//                    A stored plane begins at a multiple of 16 bytes (the pitch is one), so the loads are always aligned; an OUTPUT plane
//                    only when its first float is -- H * W % 4 == 0 guarantees it -- so a plane whose output base is not 16-byte aligned
//                    takes the scalar path: the same block of pixels, one pixel per lane and pass, 4-byte stores.  The last H * W % 4
//                    pixels of an aligned plane take it too.
// uint8 storage: image = float(u) / 255.0f, one correctly rounded division (NOT a multiply by the reciprocal: that differs at 126 of the 256
// levels); mask = 1.0f - float(m) / 255.0f, two roundings.  float32 storage: the words are copied as integers, every bit kept.
// Plain loads and stores, every output element written by exactly one thread, no atomics: bit-reproducible.
// Algorithmic bytes per camera, m = 1 with masks: (3 + m) H W read and 4 (3 + m) H W written (uint8 storage); 4 (3 + m) H W read and as many
// written (float32 storage).  Bound by memory.
#include "csplat_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CAMERA_THREADS = 256;
constexpr int CAMERA_PIXELS_PER_LANE = 16;
constexpr int CAMERA_GROUP = 4;             // pixels per 16-byte store
constexpr int CAMERA_GROUPS_PER_LANE = CAMERA_PIXELS_PER_LANE / CAMERA_GROUP;
constexpr int CAMERA_BLOCK_PIXELS = CAMERA_THREADS * CAMERA_PIXELS_PER_LANE;
constexpr int CAMERA_MAX_GRID_Z = 65535;    // cameras along z; the kernel strides over what is beyond

__device__ __forceinline__ float camera_level(unsigned u, bool is_mask) {
    const float q = (float)u / 255.0f;
    return is_mask ? 1.0f - q : q;
}

// the four pixels of one 4-byte word (little endian: the first pixel is the low byte)
__device__ __forceinline__ float4 camera_levels(unsigned w, bool is_mask) {
    float4 f;
    f.x = camera_level(w & 255u, is_mask);
    f.y = camera_level((w >> 8) & 255u, is_mask);
    f.z = camera_level((w >> 16) & 255u, is_mask);
    f.w = camera_level(w >> 24, is_mask);
    return f;
}

__global__ __launch_bounds__(CAMERA_THREADS) void k_camera_batch(int n, int64_t hw, int float_storage, int planes, int64_t n_slots, int64_t pitch,
                                                                const unsigned char *__restrict__ store, const int32_t *__restrict__ slots,
                                                                float *__restrict__ gt, float *__restrict__ mask) {
    const int p = blockIdx.y;                                   // plane of the slot: 0 .. 2 image, 3 mask
    const bool is_mask = p == 3;
    const int64_t first = (int64_t)blockIdx.x * CAMERA_BLOCK_PIXELS;          // first pixel of this block
    const int64_t last = first + CAMERA_BLOCK_PIXELS < hw ? first + CAMERA_BLOCK_PIXELS : hw;
    for (int i = blockIdx.z; i < n; i += gridDim.z) {
        float *__restrict__ out = is_mask ? mask + (int64_t)i * hw : gt + ((int64_t)i * 3 + p) * hw;
        const int64_t s = slots[i];
        if (s < 0 || s >= n_slots) {     // not a slot: the Python surface's error; every float of the camera is NaN and nothing is read
            const float nan = __builtin_nanf("");
            for (int64_t k = first + threadIdx.x; k < last; k += CAMERA_THREADS) out[k] = nan;
            continue;
        }
        const unsigned char *__restrict__ in = store + (s * planes + p) * pitch;
        const bool wide = ((uintptr_t)out & 15u) == 0;           // uniform over the workgroup
        // groups 0 .. n_groups - 1 of this block (pixels first .. full - 1) go through the wide path, pixels full .. last - 1 (the plane's
        // last H * W % 4, or everything) one by one
        const int n_groups = wide ? (int)((last - first) / CAMERA_GROUP) : 0;
        const int64_t full = first + (int64_t)n_groups * CAMERA_GROUP;
        // the lane's four groups, a pass of the workgroup apart; all four loads are issued before the first store.  (Named registers: as
        // an array indexed in unrolled loops the float32 path's four uint4 were placed in LDS.)
        static_assert(CAMERA_GROUPS_PER_LANE == 4, "four named groups per lane");
        const int g0 = threadIdx.x, g1 = g0 + CAMERA_THREADS, g2 = g1 + CAMERA_THREADS, g3 = g2 + CAMERA_THREADS;
        const bool k0 = g0 < n_groups, k1 = g1 < n_groups, k2 = g2 < n_groups, k3 = g3 < n_groups;
        if (float_storage) {
            const uint4 *__restrict__ i4 = reinterpret_cast<const uint4 *>(in + 4 * first);
            uint4 *__restrict__ o4 = reinterpret_cast<uint4 *>(out + first);
            uint4 a = make_uint4(0, 0, 0, 0), b = a, c = a, d = a;
            if (k0) a = i4[g0];
            if (k1) b = i4[g1];
            if (k2) c = i4[g2];
            if (k3) d = i4[g3];
            if (k0) o4[g0] = a;
            if (k1) o4[g1] = b;
            if (k2) o4[g2] = c;
            if (k3) o4[g3] = d;
        } else {
            const unsigned *__restrict__ i1 = reinterpret_cast<const unsigned *>(in + first);
            float4 *__restrict__ o4 = reinterpret_cast<float4 *>(out + first);
            unsigned a = 0, b = 0, c = 0, d = 0;
            if (k0) a = i1[g0];
            if (k1) b = i1[g1];
            if (k2) c = i1[g2];
            if (k3) d = i1[g3];
            if (k0) o4[g0] = camera_levels(a, is_mask);
            if (k1) o4[g1] = camera_levels(b, is_mask);
            if (k2) o4[g2] = camera_levels(c, is_mask);
            if (k3) o4[g3] = camera_levels(d, is_mask);
        }
        for (int64_t k = full + threadIdx.x; k < last; k += CAMERA_THREADS) {
            if (float_storage)
                reinterpret_cast<unsigned *>(out)[k] = reinterpret_cast<const unsigned *>(in)[k];
            else
                out[k] = camera_level(in[k], is_mask);
        }
    }
}

}  // namespace

extern "C" int csplat_camera_batch(void *stream, int n, int H, int W, int storage, int has_mask, int64_t n_slots, int64_t pitch, const void *store,
                                   const int32_t *slots, float *gt, float *mask) {
    CSPLAT_REQUIRE(n >= 0 && H >= 0 && W >= 0 && n_slots >= 0 && pitch >= 0, "csplat_camera_batch: a negative size");
    CSPLAT_REQUIRE(storage == CSPLAT_CAMERA_UINT8 || storage == CSPLAT_CAMERA_FLOAT32, "csplat_camera_batch: storage is CSPLAT_CAMERA_UINT8 or _FLOAT32");
    CSPLAT_REQUIRE(has_mask == 0 || has_mask == 1, "csplat_camera_batch: has_mask is 0 or 1");
    CSPLAT_REQUIRE(pitch % 16 == 0, "csplat_camera_batch: the pitch of a stored plane must be a multiple of 16 bytes");
    const int64_t hw = (int64_t)H * W, lim = (int64_t)1 << 31;
    CSPLAT_REQUIRE(hw < lim && n_slots < lim, "csplat_camera_batch: H * W and the number of slots must stay below 2^31");
    CSPLAT_REQUIRE(pitch >= hw * (storage == CSPLAT_CAMERA_FLOAT32 ? 4 : 1), "csplat_camera_batch: the pitch is shorter than a plane");
    if (n == 0 || hw == 0) return 0;
    CSPLAT_REQUIRE(slots && gt && (n_slots == 0 || store), "csplat_camera_batch: NULL operand");
    CSPLAT_REQUIRE((mask != nullptr) == (has_mask == 1), "csplat_camera_batch: the mask output is given exactly when the store has masks");
    CSPLAT_REQUIRE(((uintptr_t)store & 15u) == 0 && (((uintptr_t)slots | (uintptr_t)gt | (uintptr_t)mask) & 3u) == 0,
                   "csplat_camera_batch: the store must be 16-byte aligned, slots, gt and mask 4-byte aligned");
    const int planes = 3 + has_mask;
    const size_t out_bytes = (size_t)n * hw * 4, store_bytes = (size_t)n_slots * planes * pitch;
    const uintptr_t g = (uintptr_t)gt, m = (uintptr_t)mask, st = (uintptr_t)store, sl = (uintptr_t)slots;
    const auto overlap = [](uintptr_t a, size_t na, uintptr_t b, size_t nb) { return na && nb && a < b + nb && b < a + na; };
    CSPLAT_REQUIRE(!overlap(g, 3 * out_bytes, st, store_bytes) && !overlap(g, 3 * out_bytes, sl, (size_t)n * 4) &&
                       !(mask && (overlap(m, out_bytes, st, store_bytes) || overlap(m, out_bytes, sl, (size_t)n * 4) || overlap(m, out_bytes, g, 3 * out_bytes))),
                   "csplat_camera_batch: an output overlaps another operand");
    const dim3 grid((unsigned)((hw + CAMERA_BLOCK_PIXELS - 1) / CAMERA_BLOCK_PIXELS), (unsigned)planes, (unsigned)(n < CAMERA_MAX_GRID_Z ? n : CAMERA_MAX_GRID_Z));
    k_camera_batch<<<grid, CAMERA_THREADS, 0, (hipStream_t)stream>>>(n, hw, storage == CSPLAT_CAMERA_FLOAT32, planes, n_slots, pitch,
                                                                    (const unsigned char *)store, slots, gt, mask);
    LAUNCH_CHECK();
    return 0;
}
