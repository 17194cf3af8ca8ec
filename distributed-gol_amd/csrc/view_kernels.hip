// view_kernels.hip -- windowed board access on the packed torus rows: the density viewport
// (view_counts, a streaming reduction), and the rectangle codec (rect_unpack / rect_pack) behind
// golhip_store_rect / golhip_load_rect.  The engine side is engine_view.hip.
//
// Reference roles: sdl/loop.go + sdl/window.go (the window that shows the world, one pixel per
// cell) -> view_counts at a zoom where one pixel stands for a scale x scale block of cells;
// gol/io.go:42-128 (the whole world as bytes) -> the same bytes for a rectangle only.
//
// Columns: a rectangle starts at logical column x0 in [0, width) and is at most `width` wide; the
// device torus is L = wd * 32 bits, a multiple of width, so column x0 + i taken mod L is a device
// column that holds logical column (x0 + i) mod width.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "golhip_internal.hpp"

namespace golhip {
namespace {

// 4 consecutive words at a 4-byte-aligned address (one global_load_dwordx4: the global address space
// needs dword alignment only)
struct __attribute__((aligned(4))) Words4 {
    uint32_t v[4];
};

// The 4 words of bits [x0 + 128 t, x0 + 128 t + 128) of a row: device words base .. base + 4
// (base = (x0 / 32 + 4 t) mod wd, already reduced) realigned by s = x0 % 32 with v_alignbit.
// WRAP = false: the 5 words are contiguous (word 4 is read only when s != 0, from index j4, which
// the caller wrapped); WRAP = true: the one lane per row whose words straddle the end of the row
// loads them one by one.
template <bool WRAP>
__device__ __forceinline__ void load_quad(const uint32_t *__restrict__ row, int32_t base, int32_t j4, int32_t wd,
                                          int s, uint32_t (&q)[4]) {
    uint32_t d[5];
    if (!WRAP) {
        const Words4 w = *reinterpret_cast<const Words4 *>(row + base);
#pragma unroll
        for (int u = 0; u < 4; ++u) d[u] = w.v[u];
        d[4] = s ? row[j4] : 0;
    } else {
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            int32_t j = base + u;
            if (j >= wd) j -= wd;
            d[u] = row[j];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = __funnelshift_r(d[u], d[u + 1], s);
}

// acc[u] += popcount of word u of the quad, over rows [r, re): UNROLL rows' loads in flight.
template <bool WRAP, int UNROLL>
__device__ __forceinline__ void sum_rows(const uint32_t *__restrict__ row, int64_t pitch, int64_t r, int64_t re,
                                         int32_t base, int32_t wd, int s, uint32_t (&acc)[4]) {
    const int32_t j4 = base + 4 < wd ? base + 4 : 0;
    for (; r + UNROLL <= re; r += UNROLL, row += UNROLL * pitch) {
        uint32_t q[UNROLL][4];
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) load_quad<WRAP>(row + i * pitch, base, j4, wd, s, q[i]);
#pragma unroll
        for (int i = 0; i < UNROLL; ++i)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += __popc(q[i][u]);
    }
    for (; r < re; ++r, row += pitch) {
        uint32_t q[4];
        load_quad<WRAP>(row, base, j4, wd, s, q);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += __popc(q[u]);
    }
}

// view_counts, scale >= 32.  One lane owns one quad (128 columns) of one pixel row and walks the
// pixel row's `scale` board rows with a per-word popcount accumulator: 16 bytes per lane per row,
// 1 KiB contiguous per wave, kViewUnroll rows in flight.  PPQ = pixels per quad = 128 / scale for
// scale 32 / 64 (4 / 2 pixels, summed in the lane; the last quad of a pixel row may reach past the
// viewport: it reads on round the torus and stores only the pixels below w); scale >= 128 has one
// pixel per G = scale / 128 neighbouring lanes, summed by shuffles (G <= 8 divides the wave; the
// quads of a pixel row are a multiple of G, so a group of lanes is active or idle as a whole).
// Rows: `rows0` is the first of `nrows` rows this launch may read; they are rows phase .. phase +
// nrows of the launch's first pixel row onward (phase < scale), so pixel row jj covers local rows
// [jj * scale - phase, + scale) clipped to [0, nrows): partial sums where a strip or a wrap cuts
// a pixel row, added up by the host.
constexpr int kViewUnroll = 8;

template <int PPQ>
__global__ __launch_bounds__(256) void view_counts_wide(const uint32_t *__restrict__ rows0, int64_t pitch,
                                                        int64_t nrows, int32_t phase, int32_t wd, int64_t x0,
                                                        int32_t scale, int32_t w, int64_t npr,
                                                        uint32_t *__restrict__ out) {
    const int32_t nq = (int32_t)(((int64_t)w * scale + 127) >> 7);  // quads per pixel row
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= npr * nq) return;
    const int64_t jj = item / nq;
    const int32_t t = (int32_t)(item - jj * nq);
    const int s = (int)(x0 & 31);
    const int32_t base = (int32_t)(((x0 >> 5) + 4ll * t) % wd);
    int64_t r = jj * scale - phase, re = r + scale;
    if (r < 0) r = 0;
    if (re > nrows) re = nrows;
    uint32_t acc[4] = {0, 0, 0, 0};
    const uint32_t *row = rows0 + r * pitch;
    if (base + 4 <= wd)
        sum_rows<false, kViewUnroll>(row, pitch, r, re, base, wd, s, acc);
    else
        sum_rows<true, 1>(row, pitch, r, re, base, wd, s, acc);
    uint32_t *o = out + jj * w;
    if (PPQ == 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (4 * t + u < w) o[4 * t + u] = acc[u];
    } else if (PPQ == 2) {
        o[2 * t] = acc[0] + acc[1];
        if (2 * t + 1 < w) o[2 * t + 1] = acc[2] + acc[3];
    } else {
        uint32_t v = acc[0] + acc[1] + acc[2] + acc[3];
        const int G = scale >> 7;
        for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, 64);
        if ((t & (G - 1)) == 0) o[t / G] = v;
    }
}

// view_counts, scale < 32.  One lane owns one word (32 columns = PPW = 32 / scale pixels) of one
// pixel row: masked popcounts of the pixels inside the word, summed over the pixel row's rows.
template <int PPW>
__global__ __launch_bounds__(256) void view_counts_narrow(const uint32_t *__restrict__ rows0, int64_t pitch,
                                                          int64_t nrows, int32_t phase, int32_t wd, int64_t x0,
                                                          int32_t w, int64_t npr, uint32_t *__restrict__ out) {
    constexpr int kScale = 32 / PPW;
    constexpr uint32_t kMask = (1u << kScale) - 1u;
    const int32_t nw = (w + PPW - 1) / PPW;  // words per pixel row (the last may be partial)
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= npr * nw) return;
    const int64_t jj = item / nw;
    const int32_t t = (int32_t)(item - jj * nw);
    const int s = (int)(x0 & 31);
    const int32_t j0 = (int32_t)(((x0 >> 5) + t) % wd), j1 = j0 + 1 < wd ? j0 + 1 : 0;
    int64_t r = jj * kScale - phase, re = r + kScale;
    if (r < 0) r = 0;
    if (re > nrows) re = nrows;
    uint32_t acc[PPW];
#pragma unroll
    for (int p = 0; p < PPW; ++p) acc[p] = 0;
    for (; r < re; ++r) {
        const uint32_t *row = rows0 + r * pitch;
        const uint32_t v = __funnelshift_r(row[j0], row[j1], s);
#pragma unroll
        for (int p = 0; p < PPW; ++p) acc[p] += __popc((v >> (p * kScale)) & kMask);
    }
    uint32_t *o = out + jj * w + (int64_t)t * PPW;
#pragma unroll
    for (int p = 0; p < PPW; ++p)
        if (t * PPW + p < w) o[p] = acc[p];
}

// rect_unpack: columns [x0, x0 + w) of `rows` packed rows -> 0/255 bytes (compact, stride == w);
// 16 cells per thread from two adjacent words.
__global__ void rect_unpack(const uint32_t *__restrict__ row0, int64_t pitch, int64_t rows, int32_t wd,
                            int64_t x0, int64_t w, uint8_t *__restrict__ bytes) {
    const int64_t per_row = (w + 15) / 16, n = rows * per_row, L = (int64_t)wd * 32;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / per_row, i0 = (i - y * per_row) * 16;
        const int64_t c = (x0 + i0) % L;
        const int32_t j0 = (int32_t)(c >> 5), j1 = j0 + 1 < wd ? j0 + 1 : 0;
        const uint32_t *r = row0 + y * pitch;
        const uint32_t bits = __funnelshift_r(r[j0], r[j1], (int)(c & 31)) & 0xffffu;
        uint8_t *o = bytes + y * w + i0;
        if ((w & 15) == 0) {
            uint32_t q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) v |= (((bits >> (4 * k + b)) & 1u) * 0xffu) << (8 * b);
                q[k] = v;
            }
            *reinterpret_cast<uint4 *>(o) = make_uint4(q[0], q[1], q[2], q[3]);
        } else {
            for (int b = 0; b < 16 && i0 + b < w; ++b) o[b] = ((bits >> b) & 1u) ? 255 : 0;
        }
    }
}

// rect_pack: a masked read-modify-write of the device words under the rectangle.  One thread owns
// one device word (no two threads write a word), finds which of its 32 columns lie in the rectangle
// -- in whichever horizontal replica the word is -- and combines.  The words visited per row are
// words [j_first, j_first + nvis) mod wd: the rectangle's own when the torus is not replicated, the
// whole row otherwise (every replica holds a copy of the rectangle).
__global__ void rect_pack(const uint8_t *__restrict__ bytes, int64_t rows, int64_t width, int32_t wd,
                          int64_t x0, int64_t w, int32_t j_first, int32_t nvis, int mode,
                          uint32_t *__restrict__ row0, int64_t pitch) {
    const int64_t n = rows * nvis;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / nvis;
        int32_t j = j_first + (int32_t)(i - y * nvis);
        if (j >= wd) j -= wd;
        const uint8_t *src = bytes + y * w;
        int64_t k = ((int64_t)j * 32) % width - x0;  // index in the rectangle's row of the word's bit 0
        if (k < 0) k += width;
        uint32_t mask = 0, bits = 0;
        for (int b = 0; b < 32; ++b) {
            if (k < w) {
                mask |= 1u << b;
                bits |= (uint32_t)(src[k] != 0) << b;
            }
            if (++k == width) k = 0;
        }
        if (!mask) continue;
        uint32_t *p = row0 + y * pitch + j;
        const uint32_t old = *p;
        *p = mode == 0 ? (old & ~mask) | bits : mode == 1 ? old | bits : old ^ bits;
    }
}

inline unsigned blocks_for(int64_t n, int64_t cap = 8192) {
    int64_t g = (n + 255) / 256;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

}  // namespace

hipError_t launch_view_counts(const uint32_t *rows0, int64_t pitch, int64_t nrows, int32_t phase, int32_t wd,
                              int64_t x0, int32_t scale, int32_t w, int64_t npr, uint32_t *out, hipStream_t s) {
    const int64_t per_row = scale >= 32 ? ((int64_t)w * scale + 127) >> 7 : ((int64_t)w * scale + 31) >> 5;
    const int64_t items = npr * per_row;
    if (w < 1 || npr < 1 || nrows < 1 || items > (int64_t)0x7fffffff * 256) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((items + 255) / 256)), block(256);
#define GOLHIP_NARROW(PPW)                                                                                    \
    hipLaunchKernelGGL(view_counts_narrow<PPW>, grid, block, 0, s, rows0, pitch, nrows, phase, wd, x0, w, npr, out)
#define GOLHIP_WIDE(PPQ)                                                                                      \
    hipLaunchKernelGGL(view_counts_wide<PPQ>, grid, block, 0, s, rows0, pitch, nrows, phase, wd, x0, scale, w, npr, out)
    switch (scale) {
        case 1: GOLHIP_NARROW(32); break;
        case 2: GOLHIP_NARROW(16); break;
        case 4: GOLHIP_NARROW(8); break;
        case 8: GOLHIP_NARROW(4); break;
        case 16: GOLHIP_NARROW(2); break;
        case 32: GOLHIP_WIDE(4); break;
        case 64: GOLHIP_WIDE(2); break;
        case 128: case 256: case 512: case 1024: GOLHIP_WIDE(1); break;
        default: return hipErrorInvalidValue;
    }
#undef GOLHIP_NARROW
#undef GOLHIP_WIDE
    return hipGetLastError();
}

hipError_t launch_rect_unpack(const uint32_t *row0, int64_t pitch, int64_t rows, int32_t wd, int64_t x0,
                              int64_t w, uint8_t *bytes, hipStream_t s) {
    hipLaunchKernelGGL(rect_unpack, dim3(blocks_for(rows * ((w + 15) / 16))), dim3(256), 0, s, row0, pitch, rows,
                       wd, x0, w, bytes);
    return hipGetLastError();
}

hipError_t launch_rect_pack(const uint8_t *bytes, int64_t rows, int64_t width, int32_t wd, int64_t x0, int64_t w,
                            int mode, uint32_t *row0, int64_t pitch, hipStream_t s) {
    int32_t j_first = 0, nvis = wd;
    if ((int64_t)wd * 32 == width) {  // no replicas: the words the rectangle covers
        j_first = (int32_t)(x0 >> 5);
        nvis = (int32_t)std::min<int64_t>(wd, ((x0 & 31) + w + 31) >> 5);
    }
    hipLaunchKernelGGL(rect_pack, dim3(blocks_for(rows * nvis)), dim3(256), 0, s, bytes, rows, width, wd, x0, w,
                       j_first, nvis, mode, row0, pitch);
    return hipGetLastError();
}

}  // namespace golhip
