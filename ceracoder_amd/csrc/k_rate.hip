// k_rate.hip -- frame-rate conversion: the mix of two pictures at a tick's instant.  One elementwise launch over the whole coded NV12
// surfaces of a slot, W x H x 3/2 bytes, margins included: both inputs' margins are replicas of their last visible row / column, and the mix is taken sample by
// sample, so the mix of the margins is the replica of the mix.
//
//   out = (a (256 - w) + b w + 128) >> 8      per byte, luma and chroma alike; w = 0 .. 256 (0 and 256 give a and b exactly: 256 a + 128 >> 8 = a)
//
// A lane takes 16 bytes of each source and stores 16 bytes.  The arithmetic runs on packed bytes, two 16-bit lanes per dword: the even bytes of a dword
// (x & 0x00FF00FF) and the odd ones ((x >> 8) & 0x00FF00FF) are two 16-bit fields each, and a field's value a (256 - w) + b w + 128 <= 255 * 256 + 128 < 2^16
// never carries into its neighbour -- so one 32-bit multiply-add handles two samples, and the two results are put together by mask and shift.
// With `keep` the lane also stores the b it read at the same index of the keep buffer.  In the encoder a == keep and b == out (the mix lands in the slot, the
// slot's input in the keep buffer): the lane that reads an index is the only one that writes it, and it has read both sources before its first store, so the
// launch works in place.  No LDS, no atomics, no scratch, no wait.
#include "kernels_common.hpp"

struct rate_args {
    const uint4 *a_y, *a_uv, *b_y, *b_uv; // the previous input (the keep buffer) and this one
    uint4 *o_y, *o_uv;                    // the tick's slot
    uint4 *k_y, *k_uv;                    // null: b is not kept
    unsigned ny, n;                       // 16-byte words of the luma surface / of both surfaces
    unsigned w;                           // 0 .. 256
};

DEV unsigned mix_dword(unsigned a, unsigned b, unsigned wa, unsigned wb) {
    const unsigned m = 0x00FF00FFu, half = 0x00800080u;
    // (the masked operands have 24 bits and the weights 9: the 24-bit multiply's low 32 bits are the whole product, at the full VALU rate)
    const unsigned e = (__umul24(a & m, wa) + __umul24(b & m, wb) + half) >> 8;      // even bytes: results in bits 0 .. 7 and 16 .. 23
    const unsigned o = __umul24((a >> 8) & m, wa) + __umul24((b >> 8) & m, wb) + half; // odd bytes: results in bits 8 .. 15 and 24 .. 31
    return (e & m) | (o & ~m);
}

__global__ __launch_bounds__(256) void rate_mix_kernel(rate_args g) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= g.n) return;
    const bool luma = i < g.ny;
    const unsigned j = luma ? i : i - g.ny;
    const uint4 a = (luma ? g.a_y : g.a_uv)[j], b = (luma ? g.b_y : g.b_uv)[j];
    const unsigned wb = g.w, wa = 256u - g.w;
    uint4 r;
    r.x = mix_dword(a.x, b.x, wa, wb); r.y = mix_dword(a.y, b.y, wa, wb);
    r.z = mix_dword(a.z, b.z, wa, wb); r.w = mix_dword(a.w, b.w, wa, wb);
    (luma ? g.o_y : g.o_uv)[j] = r;
    if (g.k_y) (luma ? g.k_y : g.k_uv)[j] = b;
}

// surfaces of W x H and W x H / 2 bytes at stride W (W, H multiples of 16), every pointer 16-byte aligned; -1: arguments outside that
int k_launch_rate_mix(const uint8_t *a_y, const uint8_t *a_uv, const uint8_t *b_y, const uint8_t *b_uv, uint8_t *o_y, uint8_t *o_uv, uint8_t *k_y, uint8_t *k_uv,
                      int W, int H, int w256, hipStream_t s) {
    if (W < 16 || H < 16 || (W & 15) || (H & 15) || w256 < 0 || w256 > 256 || !a_y || !a_uv || !b_y || !b_uv || !o_y || !o_uv || !k_y != !k_uv) return -1;
    if ((((uintptr_t)a_y | (uintptr_t)a_uv | (uintptr_t)b_y | (uintptr_t)b_uv | (uintptr_t)o_y | (uintptr_t)o_uv | (uintptr_t)k_y | (uintptr_t)k_uv) & 15) != 0) return -1;
    rate_args g;
    g.a_y = (const uint4 *)a_y; g.a_uv = (const uint4 *)a_uv; g.b_y = (const uint4 *)b_y; g.b_uv = (const uint4 *)b_uv;
    g.o_y = (uint4 *)o_y; g.o_uv = (uint4 *)o_uv; g.k_y = (uint4 *)k_y; g.k_uv = (uint4 *)k_uv;
    const size_t ny = (size_t)W * H / 16;
    g.ny = (unsigned)ny; g.n = (unsigned)(ny + ny / 2); g.w = (unsigned)w256;
    hipLaunchKernelGGL(rate_mix_kernel, dim3((g.n + 255u) / 256u), dim3(256), 0, s, g);
    return 0;
}
