// batch_board.hip -- gol_batch: MANY independent small tori in one launch, one workgroup each.
//
// gol_board (stencil_board.hip) holds a whole torus of at most 512 x 512 cells in one workgroup's
// registers and leaves the other 255 CUs idle.  People who run small tori run thousands of them
// (soup searches, seed and density sweeps, censuses of what a board settles to), so here
// blockIdx.x selects the board: board i lives at boards + i * board_pitch words, in the packed
// layout of a single engine of that size (rows of wd in {4, 8, 16} words, pitch wd).  The geometry
// is gol_board's (board_common.hpp): W waves, four 16-lane DPP segments per wave, R rows per
// segment in VGPRs, row_ror:1 for the torus wrap, and gol_board's generation step: sums16, then
// board_gen (the segments' edge-row sums through LDS under one LDS-only barrier per generation);
// K (runtime, <= kBoardMaxK) generations per launch, unrotate16 on the way out.  No trapezoid, no
// halo, no inter-workgroup traffic.  gol_batch_rule (batch_rule.hpp) keeps a copy of this kernel's
// body around the same board_gen: with the two bodies folded into one inlined function the HIST
// kernels here got another prologue and their calls took up to 6 % longer.
//
// A workgroup reads its whole board into registers before it stores anything and every wave
// stores exactly the rows it loaded, so a launch advances the boards IN PLACE: no second buffer.
//
// HIST: the alive count of board i after each generation g of the launch, hist[i * K + g]
// (uint32).  W waves contribute to a count.  Generations run in groups of 4 as in gol_board (the
// four 6-step wave reductions interleave after the group); lane 63 of each wave then puts its 4
// partial sums into LDS, cnt[group parity][u][w].  The NEXT group's barriers order those stores
// before wave 0 reads them at that group's end: lane 16 u + j takes cnt[..][u][j] (0 for j >= W),
// four row_shr adds leave the sum of generation u in lane 16 u + 15, which stores it.  One
// ds_write per wave, and on wave 0 one ds_read, 4 DPP adds and one global store, per FOUR
// generations; no atomics, no extra barrier (one at the very end for the last group), no
// finalize pass, and the result is a plain store: hist needs no zeroing.  The buffer parity is
// safe: group G + 2 overwrites cnt[G & 1] only after its own barriers, which wave 0 reaches after
// its read of group G (the LDS barrier waits lgkmcnt(0) first).
//
// SETTLE: each lane keeps board(t - 1) of its rows (R more VGPRs) beside board(t) and, once
// board(t + 1) is computed, compares the two.  The frame drifts one bit east per generation, so
// board(t - 1) has to move two bits east: the first bit is free -- sums16's ctr IS the row moved one
// bit east, and that is what the lane keeps -- the second is one DPP and one v_alignbit a
// generation later; one v_bitop3 OR-s the XOR into an accumulator: 3 VALU per word per generation.  No agreement across waves per generation: B3/S23
// is deterministic, so board(t) == board(t - 2) holds for every later t once it holds, and a lane
// only records the LAST turn at which any of its rows differed from two turns before; the
// board's settle turn is 1 + the maximum of that over lanes, waves, launches and calls.  The
// kernel reduces it over the wave once at the end and takes one atomicMax per wave on
// last_diff[board] (absolute turns, so the engine combines launches by doing nothing).  board(t0 - 1)
// comes from, and board(t0 + K - 1) goes to, prev (same layout as boards, also in place); at
// t0 == 0 there is no board(-1) and the first generation compares nothing.
#include "board_common.hpp"

namespace golhip {
namespace {

template <int W, int R, bool HIST, bool SETTLE>
__global__ __launch_bounds__(64 * W) void gol_batch(BatchParams p, int K) {
    constexpr int NSEG = 4 * W;
    __shared__ uint32_t ex[2][NSEG][4][16];
    __shared__ uint32_t cnt[2][4][16];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c16 = lane & 15;
    const int sg = 4 * w + (lane >> 4);
    const int wd = p.wd;
    const bool own = c16 < wd;  // one copy of the replicated row is stored
    // HIST counts one copy of the BOARD's row: `width` consecutive bits of the row, which has period
    // `width`, hold every cell once in any drifted frame
    const int cw = (p.width + 31) >> 5;
    const uint32_t cmask = c16 >= cw ? 0u : (c16 == cw - 1 && (p.width & 31)) ? (1u << (p.width & 31)) - 1u : ~0u;
    const int64_t boff = (int64_t)blockIdx.x * p.board_pitch;
    uint32_t *__restrict__ board = p.boards + boff;
    uint32_t c[R];
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = board[(sg * R + r) * wd + (c16 & (wd - 1))];
    // SETTLE: board(t - 1) in board(t)'s frame; at t0 == 0 there is none
    uint32_t old[SETTLE ? R : 1];
    uint32_t last = 0;  // 1 + the last generation of this launch whose result differed (0: none)
    const int gmin = p.t0 > 0 ? 0 : 1;
    if constexpr (SETTLE) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            old[r] = gmin == 0 ? p.prev[boff + (sg * R + r) * wd + (c16 & (wd - 1))] : 0u;
        }
    }
    const int up = (sg + NSEG - 1) % NSEG, dn = (sg + 1) % NSEG;
    // generation g (exchange buffer par): the rows advance in place; returns this lane's alive
    // cells of the new generation (HIST)
    auto gen = [&](int g, int par) -> uint32_t {
        uint32_t s[R], cy[R], ctr[R], nx[R];
        sums16<R>(c, s, cy, ctr);
        board_gen<R>(s, cy, ctr, ex, par, sg, up, dn, c16, LifeNext{}, nx);
        uint32_t a = 0;
        if constexpr (HIST)
#pragma unroll
            for (int r = 0; r < R; ++r) a += (uint32_t)__builtin_popcount(nx[r] & cmask);
        if constexpr (SETTLE) {
            uint32_t wl[R], e1[R], acc = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) wl[r] = west16(old[r]);
#pragma unroll
            for (int r = 0; r < R; ++r) e1[r] = __builtin_amdgcn_alignbit(old[r], wl[r], 31);  // one more bit east
#pragma unroll
            for (int r = 0; r < R; ++r) acc = GOL_BOP3(acc, nx[r], e1[r], GOL_TT(a | (b ^ c)));
            if (acc != 0 && g >= gmin) last = (uint32_t)g + 1;
            // pin the compare to its generation: left free, the compiler sinks the four compares of a
            // group behind its last barrier and keeps every generation's rows alive until then
            asm volatile("" : "+v"(last));
#pragma unroll
            for (int r = 0; r < R; ++r) old[r] = ctr[r];  // board(t) in board(t + 1)'s frame, from sums16
        }
#pragma unroll
        for (int r = 0; r < R; ++r) c[r] = nx[r];
        return a;
    };
    // HIST: wave 0 sums the W partials of the n generations from g0 that lie in cnt[buf]
    auto flush = [&](int buf, int g0, int n) {
        if (w == 0) {
            const int u = lane >> 4;
            uint32_t v = c16 < W ? cnt[buf][u][c16] : 0u;
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
            if (c16 == 15 && u < n) p.hist[(int64_t)blockIdx.x * K + g0 + u] = v;
        }
    };
    int g = 0, grp = 0;
#pragma clang loop unroll(disable)
    for (; g + 4 <= K; g += 4, ++grp) {
        uint32_t a[4];
        a[0] = gen(g, 0);
        a[1] = gen(g + 1, 1);
        a[2] = gen(g + 2, 0);
        a[3] = gen(g + 3, 1);
        if constexpr (HIST) {
            wave_sum_dpp_n<4>(a);
            if (grp > 0) flush((grp - 1) & 1, g - 4, 4);
            if (lane == 63)
#pragma unroll
                for (int u = 0; u < 4; ++u) cnt[grp & 1][u][w] = a[u];
        }
    }
    const int rem = K - g;  // 0..3 generations left: one more, partial, group
    if (rem > 0) {
        uint32_t a[4] = {0, 0, 0, 0};
        a[0] = gen(g, 0);
        if (rem > 1) a[1] = gen(g + 1, 1);
        if (rem > 2) a[2] = gen(g + 2, 0);
        if constexpr (HIST) {
            wave_sum_dpp_n<4>(a);
            if (grp > 0) flush((grp - 1) & 1, g - 4, 4);
            if (lane == 63)
#pragma unroll
                for (int u = 0; u < 4; ++u) cnt[grp & 1][u][w] = a[u];
        }
        ++grp;
    }
    if constexpr (HIST) {  // the last group's partials: one more barrier orders them
        lds_barrier();
        flush((grp - 1) & 1, (grp - 1) * 4, rem > 0 ? rem : 4);
    }
    // the rows back in the board frame (K bits west around the torus), one copy stored
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t v = unrotate16(c[r], lane, K);
        if (own) board[(sg * R + r) * wd + c16] = v;
        if constexpr (SETTLE) {
            const uint32_t o = unrotate16(old[r], lane, K);
            if (own) p.prev[boff + (sg * R + r) * wd + c16] = o;
        }
    }
    if constexpr (SETTLE) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) last = max(last, (uint32_t)__shfl_xor((int)last, off, 64));
        if (lane == 0 && last)
            atomicMax(&p.last_diff[blockIdx.x], (unsigned long long)p.t0 + (unsigned long long)last);
    }
}

template <int W, int R>
hipError_t launch_batch_wr(int K, int nboards, const BatchParams &p, hipStream_t s) {
    const bool hist = p.hist != nullptr, settle = p.prev != nullptr;
    const dim3 grid((unsigned)nboards), block(64 * W);
    if (hist && settle)
        hipLaunchKernelGGL((gol_batch<W, R, true, true>), grid, block, 0, s, p, K);
    else if (hist)
        hipLaunchKernelGGL((gol_batch<W, R, true, false>), grid, block, 0, s, p, K);
    else if (settle)
        hipLaunchKernelGGL((gol_batch<W, R, false, true>), grid, block, 0, s, p, K);
    else
        hipLaunchKernelGGL((gol_batch<W, R, false, false>), grid, block, 0, s, p, K);
    return hipGetLastError();
}

// init_random_rows (golhip_kernels.hip) for every board of a batch: word for word what a single
// engine of that size gets from seed_i = seeds ? seeds[i] : seed0 + i.
__global__ void batch_init_random(uint32_t *__restrict__ boards, int64_t board_pitch, int64_t nboards, int64_t rows,
                                  int64_t width, int32_t wd, const uint64_t *__restrict__ seeds, uint64_t seed0,
                                  uint32_t density) {
    const uint64_t g = 0x9E3779B97F4A7C15ULL;
    const int64_t per = rows * wd, n = nboards * per, wpr = width / 64;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bi = i / per, ib = i - bi * per;
        const int64_t y = ib / wd;
        const int32_t col = (int32_t)(ib - y * wd);
        const uint64_t seed = seeds ? seeds[bi] : seed0 + (uint64_t)bi;
        const int64_t x0 = ((int64_t)col * 32) % width;
        uint32_t v = 0;
        if (density == 0x80000000u) {
            const uint64_t wi = (uint64_t)y * wpr + (uint64_t)(x0 >> 6);
            const uint64_t wv = splitmix64(seed + (wi + 1) * g);
            v = (x0 & 32) ? (uint32_t)(wv >> 32) : (uint32_t)wv;
        } else {
            for (int b = 0; b < 32; ++b) {
                const uint64_t cell = (uint64_t)y * width + (uint64_t)(x0 + b);
                const uint32_t d = (uint32_t)splitmix64(seed + (cell + 1) * g);
                v |= (uint32_t)(d < density) << b;
            }
        }
        boards[bi * board_pitch + ib] = v;
    }
}

// Alive cells of each board: one wave per board, the first `cw` words of each row of wd words
// (one copy of a replicated row).
__global__ void batch_popcount(const uint32_t *__restrict__ boards, int64_t board_pitch, int64_t nboards,
                               int64_t rows, int32_t wd, int32_t cw, uint32_t tailmask, uint32_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t per = rows * wd;
    for (int64_t bi = wave; bi < nboards; bi += nwaves) {
        uint32_t a = 0;
        for (int64_t i = lane; i < per; i += 64) {
            const int32_t col = (int32_t)(i % wd);
            uint32_t v = col < cw ? boards[bi * board_pitch + i] : 0u;
            if (col == cw - 1) v &= tailmask;
            a += (uint32_t)__builtin_popcount(v);
        }
        a = wave_sum_dpp(a);
        if (lane == 63) out[bi] = a;
    }
}

unsigned batch_grid(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 1 << 16); }

}  // namespace

hipError_t launch_batch_board(int K, int W, int R, int nboards, const BatchParams &p, hipStream_t s) {
    if (K < 1 || K > kBoardMaxK || nboards < 1 || p.board_pitch != (int64_t)4 * W * R * p.wd ||
        (p.wd != 4 && p.wd != 8 && p.wd != 16) || (p.prev && !p.last_diff))
        return hipErrorInvalidValue;
#define GOLHIP_X(WW, RR) \
    if (W == WW && R == RR) return launch_batch_wr<WW, RR>(K, nboards, p, s);
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

hipError_t launch_batch_init_random(uint32_t *boards, int64_t board_pitch, int64_t nboards, int64_t rows,
                                    int64_t width, int32_t wd, const uint64_t *seeds, uint64_t seed0,
                                    uint32_t density_q32, hipStream_t s) {
    hipLaunchKernelGGL(batch_init_random, dim3(batch_grid(nboards * rows * wd)), dim3(256), 0, s, boards, board_pitch,
                       nboards, rows, width, wd, seeds, seed0, density_q32);
    return hipGetLastError();
}

hipError_t launch_batch_popcount(const uint32_t *boards, int64_t board_pitch, int64_t nboards, int64_t rows,
                                 int64_t width, int32_t wd, uint32_t *out, hipStream_t s) {
    // one copy of the replicated row: the first ceil(width / 32) words, the last one masked
    const int32_t cw = (int32_t)((width + 31) / 32);
    const uint32_t tailmask = (width & 31) ? ((1u << (width & 31)) - 1u) : 0xffffffffu;
    hipLaunchKernelGGL(batch_popcount, dim3(batch_grid(nboards * 64)), dim3(256), 0, s, boards, board_pitch, nboards,
                       rows, wd, cw, tailmask, out);
    return hipGetLastError();
}

}  // namespace golhip
