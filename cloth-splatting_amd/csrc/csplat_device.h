// csplat_device.h -- device-side helpers shared by the .hip files (gfx950, wave64); csplat_common.h is the host side.
// The library's "fixed order, bit-reproducible" sums are made of the two reductions below: their order is stated here once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) < __builtin_inff(); }      // (false for a NaN)

// ---- wave reduction: an xor butterfly over the offsets WIDTH/2, WIDTH/4 .. 1, in that order, inside every aligned group of WIDTH
// lanes; each lane of a group ends with the group's result, formed in the same order.  float, double, int, uint32_t
struct OpSum {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMin {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
    __device__ __forceinline__ int operator()(int a, int b) const { return a < b ? a : b; }
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; }
};
struct OpMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
    __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; }
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};
// (`_each`: several quantities, of any of these types, take each step of the butterfly together)
template <int WIDTH = 64, typename Op, typename... T>
__device__ __forceinline__ void wave_reduce_each(Op op, T &...v) {
    static_assert(WIDTH >= 2 && WIDTH <= 64 && (WIDTH & (WIDTH - 1)) == 0, "a power of two of lanes inside one wave");
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) ((v = op(v, __shfl_xor(v, o, 64))), ...);
}
template <int WIDTH = 64, typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
    wave_reduce_each<WIDTH>(op, v);
    return v;
}
template <int WIDTH = 64, typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce<WIDTH>(v, OpSum{}); }
template <int WIDTH = 64, typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce<WIDTH>(v, OpMin{}); }
template <int WIDTH = 64, typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce<WIDTH>(v, OpMax{}); }
template <int WIDTH = 64, typename... T> __device__ __forceinline__ void wave_sum_each(T &...v) { wave_reduce_each<WIDTH>(OpSum{}, v...); }

// ---- block reduction of a workgroup of THREADS lanes (a multiple of 64) through THREADS / 64 LDS slots per quantity, which the caller
// declares: lane 0 of wave w stashes its wave's result in slot w; after ONE barrier, whatever the number and the types of the
// quantities, a thread joins the slots in wave order, starting from the identity.  Every thread that joins gets the same bits.
__device__ __forceinline__ void block_put(int) {}
template <typename T, typename... More>
__device__ __forceinline__ void block_put(int wave, T *slots, T wave_result, More... more) {
    slots[wave] = wave_result;
    block_put(wave, more...);
}
template <typename... SlotsThenResult>
__device__ __forceinline__ void block_stash(SlotsThenResult... pairs) {      // block_stash(s_a, a, s_b, b): one branch for all of them
    if ((threadIdx.x & 63) == 0) block_put(threadIdx.x >> 6, pairs...);
}
template <int THREADS, typename T, typename Op>
__device__ __forceinline__ T block_join(const T *slots, T identity, Op op) {
    T t = identity;
    for (int k = 0; k < THREADS / 64; k++) t = op(t, slots[k]);
    return t;
}
// the common case in one call: each v becomes the workgroup's sum of it -- in thread 0 only, or in EVERY thread; the others keep their
// wave's sum.  N quantities of one type through slots[N][THREADS / 64], row m for the m-th (one quantity: a plain [THREADS / 64] array)
template <int THREADS, bool EVERY = false, typename T, int N, typename... V>
__device__ __forceinline__ void block_sum(T (&slots)[N][THREADS / 64], V &...v) {
    static_assert(N == sizeof...(V), "one row of slots per quantity");
    wave_sum_each(v...);
    int m = 0;
    if ((threadIdx.x & 63) == 0) (block_put(threadIdx.x >> 6, slots[m++], v), ...);
    __syncthreads();
    m = 0;
    if (EVERY || threadIdx.x == 0) ((v = block_join<THREADS>(slots[m++], T(0), OpSum{})), ...);
}
template <int THREADS, bool EVERY = false, typename T>
__device__ __forceinline__ void block_sum(T (&slots)[THREADS / 64], T &v) {
    block_sum<THREADS, EVERY>(reinterpret_cast<T (&)[1][THREADS / 64]>(slots), v);
}

// ---- gaussian_renderer._project: [x y z 1] @ full (row-vector convention, `full` row-major as torch stores it), /w, ndc -> pixel
// (pixel centres at the integers).  Unused fields cost nothing
struct PixelProj { float x, y, w, ndx, ndy; };
__device__ __forceinline__ PixelProj project_pixel(float x, float y, float z, const float *__restrict__ full, float W, float H) {
    PixelProj p;
    const float hx = x * full[0] + y * full[4] + z * full[8] + full[12];
    const float hy = x * full[1] + y * full[5] + z * full[9] + full[13];
    p.w = x * full[3] + y * full[7] + z * full[11] + full[15];
    p.ndx = hx / p.w;
    p.ndy = hy / p.w;
    p.x = ((p.ndx + 1.f) * W - 1.f) * 0.5f;
    p.y = ((p.ndy + 1.f) * H - 1.f) * 0.5f;
    return p;
}
