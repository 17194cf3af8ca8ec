// batch_objects.hpp -- gol_batch_objects: every cluster of live cells of every board of a batch, with its
// position, extent, population and a shape hash that no translation, rotation or reflection changes
// (golhip_batch_objects, include/golhip.h states the definitions).  ONE kernel: width, height,
// topology, reach and the cap are run-time values, as in the census kernel (batch_census.hpp), and for the same reason:
// it steps no generation, and the production library has a size to keep (tests/test_boundary.py).
//
// One workgroup per board, blockIdx.x = the board within the launch.  Dynamic LDS holds two bitmaps of
// the board's shape, H rows of nw = max(1, width / 32) words, and a block of sums:
//   R  the cells that remain: the board, bits at columns >= width cleared, minus the clusters done
//   F  the cluster being flooded
// Neither has margins.  A neighbouring row or word is found by index: wrapped on a torus, left out on
// a plane.  A row narrower than a word keeps its `width` bits in R and F; on a torus the flood
// replicates the word it has read over all 32 bits, so that one v_alignbit sees the wrap.
//
// The clusters come out in the order of the definition because the seed of each is the first set bit of
// R in row-major order, which is word order and then bit order: a lane's candidate is the first
// nonzero word among its own (i = tid, tid + blockDim, ...), the wave's is a DPP min ladder, and lane
// 63 of each wave does one ds_min_u32 on the seed slot.
//
// Per cluster:
//   init     F = the seed bit alone; the cluster's block of sums zeroed; the NEXT seed slot set to none
//   flood    F <- (F | dilate(F, reach)) & R until a whole pass changes nothing.  A lane looks only at
//            words where R has a cell F has not; it ORs the rows within `reach` of its word and of the
//            two words beside it, dilates once horizontally (v_alignbit by 31, 1, 30, 2), and then
//            goes on inside its own word in registers until that stops changing.  F is updated in
//            place: the flood is monotone (bits are only set, and only bits of the cluster), so a
//            lane that reads a neighbour's old word instead of its new one only learns later what it
//            would have learnt now.  The pass that ends the flood changed nothing, so every word
//            was read as it finally is, and F is the fixed point: the cluster.
//   pass 1   popcount, the column occupancy (ds_or_b32 of the word itself into its column word), the
//            row occupancy (one bit per row), R <- R & ~F, and the candidate for the next seed
//   extent   by every lane from the occupancy words (at most 16 per axis, broadcast reads): a start
//            is an occupied column with `reach` empty ones before it, an end one with `reach` empty
//            ones after it, both by v_alignbit against the neighbouring word; no per-column loop.
//            No start: the cluster winds.
//   hash     a lane walks the set bits of its words of F with ctz and adds mix() of the cell's place in
//            each of the eight orientations to eight 64-bit sums; a wave that holds a cell of the
//            cluster reduces them with the DPP ladder (two DPP moves and one 64-bit add per step)
//            and lane 63 does one ds_add_u64 per sum.  Sums mod 2^64 do not depend on the order.
//   record   thread 0 XORs in the box terms, takes the smallest H_k and writes the 32 bytes with plain
//            vector stores, if the cluster's number lies in the launch's window and below the cap.
// Past the cap, or without a record buffer, extent and hash are skipped and the count goes on.
//
// The barrier argument.  The trip counts of the cluster loop and of the flood loop depend on the
// board, and every __syncthreads below sits inside one or both.  No wave may take a different number of
// trips than the others, so each continue-or-stop decision is ONE value in LDS that every wave reads
// after a barrier, made wave-uniform with readfirstlane before the branch; none is a ballot.
//   - The cluster loop goes on while the seed slot of the cluster's parity is not `none`.  The slot
//     is written in the previous cluster's init (none) and pass 1 (ds_min), both before that
//     cluster's barrier C; it is read after barrier D by every wave and written again only in the
//     init of the cluster after this one, which no wave reaches before every wave has passed this
//     cluster's barrier B -- behind its read.  The first slot is ordered by the two barriers of the
//     staging in the same way.
//   - The flood loop goes on while chg[it % 3] is nonzero.  Lanes store 1 there in pass `it`, before
//     the pass's barrier; every wave reads it after that barrier.  Thread 0 clears chg[(it + 1) % 3]
//     before the same barrier: its last readers read it after barrier it - 2 and have since arrived
//     at barrier it - 1, and its next writers come after barrier `it`.  With two slots a slow wave
//     could still be reading the slot a fast one clears, hence three.
//   - `want`, which guards extent and hash but no barrier, comes from kernel arguments and the
//     cluster's number.
//   - Both loops also end by a bound that holds whatever LDS says: a pass that changes something
//     sets a bit of F and a cluster takes a bit from R, so nwords * 32 trips are never exceeded.
// The sums are double-buffered by the cluster's parity: thread 0 reads cluster c's block after
// barrier D while the other waves already zero cluster c + 1's, the other block; block c & 1 is
// zeroed again in the init of cluster c + 2, behind three barriers thread 0 has to arrive at first.
// The DPP ladders run where the wave is converged (behind the lane loops, block sizes are multiples
// of 64); the per-wave ballot in the hash encloses DPP moves and LDS atomics, no barrier.
//
// Bounds.  Board reads: row y < height, word k < nw <= wd, inside the board's pitch.  R and F: index
// (yy & (H - 1)) * nw + (k' & (nw - 1)) < nwords.  Occupancy words: k < 16 and y >> 5 < 16 (width and
// height <= 512).  The record index is count - first with first <= count < first + window.  The launcher
// refuses shapes the engine cannot have made.
//
// Size.  This header includes golhip_internal.hpp only, as batch_census.hpp does and for its reason:
// the object carries no helper kernel.  The DPP ladders are written out here.
#pragma once
#include "golhip_internal.hpp"

namespace golhip {
namespace {

constexpr uint32_t kObjNone = 0xFFFFFFFFu;  // no cell: above every cell index (512 * 512 at most)
// a cluster's block of sums in LDS, in words: eight 64-bit sums, the population, the seed of the
// cluster that uses the block, the column and row occupancy; two blocks, then chg[3]
constexpr int kObjSum = 0, kObjPop = 16, kObjSeed = 17, kObjOccX = 18, kObjOccY = 34, kObjBlk = 52;
constexpr int kObjChg = 2 * kObjBlk, kObjCtrl = 2 * kObjBlk + 4;  // 432 bytes: R starts 16-byte aligned

// the sum of v over the wave's 64 lanes, in lane 63 (wave_sum_dpp's six steps, golhip_stencil.hpp)
__device__ __forceinline__ uint32_t objects_wave_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
    return v;
}
// the same ladder on 64-bit sums: the halves move separately, the add carries
#define GOLHIP_OBJ_SUM64_STEP(ctrl, rows)                                                                        \
    v += ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, rows, 0xf, false) << 32) | \
         (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, rows, 0xf, false)
__device__ __forceinline__ uint64_t objects_wave_sum64(uint64_t v) {
    GOLHIP_OBJ_SUM64_STEP(0x111, 0xf);
    GOLHIP_OBJ_SUM64_STEP(0x112, 0xf);
    GOLHIP_OBJ_SUM64_STEP(0x114, 0xf);
    GOLHIP_OBJ_SUM64_STEP(0x118, 0xf);
    GOLHIP_OBJ_SUM64_STEP(0x142, 0xa);
    GOLHIP_OBJ_SUM64_STEP(0x143, 0xc);
    return v;
}
#undef GOLHIP_OBJ_SUM64_STEP
// the minimum of v over the wave, in lane 63: a lane the step does not reach keeps `old`, its own value
#define GOLHIP_OBJ_MIN_STEP(ctrl, rows)                                                                          \
    {                                                                                                            \
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rows, 0xf, false);         \
        v = o < v ? o : v;                                                                                       \
    }
__device__ __forceinline__ uint32_t objects_wave_min(uint32_t v) {
    GOLHIP_OBJ_MIN_STEP(0x111, 0xf)
    GOLHIP_OBJ_MIN_STEP(0x112, 0xf)
    GOLHIP_OBJ_MIN_STEP(0x114, 0xf)
    GOLHIP_OBJ_MIN_STEP(0x118, 0xf)
    GOLHIP_OBJ_MIN_STEP(0x142, 0xa)
    GOLHIP_OBJ_MIN_STEP(0x143, 0xc)
    return v;
}
#undef GOLHIP_OBJ_MIN_STEP

// mix(v) of include/golhip.h: the splitmix64 finaliser
__device__ __forceinline__ uint64_t objects_mix(uint64_t v) {
    uint64_t z = v + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The extent along one axis from its occupancy (`len` bits in len / 32 words, one word below 32; occ is
// LDS).  A start is an occupied place with `reach` empty ones before it, an end one with `reach`
// empty ones after it; cyclic (a torus) the word before the first is the last, and an occupancy
// narrower than a word is replicated over the word so that the shifts wrap.  A connected cluster has
// one start and one end, or, cyclic, none: then it winds (true), x0 = 0 and w = len.
__device__ __forceinline__ bool objects_extent(const uint32_t *occ, int len, bool cyclic, int reach, int &x0, int &w) {
    const int n = len >= 32 ? len >> 5 : 1;
    const uint32_t mask = len >= 32 ? ~0u : (1u << len) - 1u;
    int sp = -1, ep = 0;
    for (int k = 0; k < n; ++k) {
        uint32_t o = occ[k];
        uint32_t p = cyclic || k > 0 ? occ[(k - 1) & (n - 1)] : 0u;
        uint32_t nx = cyclic || k < n - 1 ? occ[(k + 1) & (n - 1)] : 0u;
        if (len < 32 && cyclic) {
            for (int s = len; s < 32; s <<= 1) o |= o << s;
            p = nx = o;
        }
        uint32_t before = __builtin_amdgcn_alignbit(o, p, 31), after = __builtin_amdgcn_alignbit(nx, o, 1);
        if (reach == 2) {
            before |= __builtin_amdgcn_alignbit(o, p, 30);
            after |= __builtin_amdgcn_alignbit(nx, o, 2);
        }
        const uint32_t st = o & ~before & mask, en = o & ~after & mask;
        if (st) sp = 32 * k + __builtin_ctz(st);
        if (en) ep = 32 * k + __builtin_ctz(en);
    }
    if (sp < 0) {
        x0 = 0;
        w = len;
        return true;
    }
    x0 = sp;
    w = ((ep - sp) & (len - 1)) + 1;
    return false;
}

__global__ __launch_bounds__(1024) void gol_batch_objects(const uint32_t *__restrict__ boards, int64_t board_pitch,
                                                          int32_t wd, int32_t width, int32_t height, int32_t plane,
                                                          int32_t reach, int32_t max_objects, int32_t first,
                                                          int32_t window, int32_t *__restrict__ nobjects,
                                                          ObjectRecord *__restrict__ objects) {
    extern __shared__ __attribute__((aligned(16))) uint32_t objects_lds[];
    const int tid = (int)threadIdx.x, nthreads = (int)blockDim.x, lane = tid & 63;
    const int H = height;
    const int nw = width >= 32 ? width >> 5 : 1;  // a power of two, as H is
    const int lgnw = 31 - __builtin_clz((unsigned)nw), nwords = H << lgnw;
    const uint32_t wmask = width >= 32 ? ~0u : (1u << width) - 1u;
    uint32_t *chg = objects_lds + kObjChg, *Rm = objects_lds + kObjCtrl, *Fm = Rm + nwords;
    const uint32_t *board = boards + (int64_t)blockIdx.x * board_pitch;

    // the board into R, and the first seed
    if (tid == 0) objects_lds[kObjSeed] = kObjNone;
    uint32_t cand = kObjNone;
    #pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = tid; i < nwords; i += nthreads) {
        const uint32_t v = board[(i >> lgnw) * wd + (i & (nw - 1))] & wmask;
        Rm[i] = v;
        if (v && cand == kObjNone) cand = (uint32_t)i * 32u + (uint32_t)__builtin_ctz(v);
    }
    __syncthreads();
    cand = objects_wave_min(cand);
    if (lane == 63 && cand != kObjNone) atomicMin(&objects_lds[kObjSeed], cand);
    __syncthreads();

    const int most = nwords * 32;  // cells: no board has more clusters, no flood more passes
    int count = 0;
    for (; count < most; ++count) {
        uint32_t *st = objects_lds + (count & 1) * kObjBlk, *nx = objects_lds + ((count & 1) ^ 1) * kObjBlk;
        const uint32_t seed = (uint32_t)__builtin_amdgcn_readfirstlane((int)st[kObjSeed]);
        if (seed == kObjNone) break;  // one value, read by every wave behind a barrier
        const bool want = objects != nullptr && count >= first && count - first < window && count < max_objects;

        // init
        #pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int i = tid; i < nwords; i += nthreads) Fm[i] = (uint32_t)i == seed >> 5 ? 1u << (seed & 31u) : 0u;
                if (tid < kObjBlk && tid != kObjSeed) st[tid] = 0;  // a block is smaller than a wave
        if (tid == 0) {
            nx[kObjSeed] = kObjNone;
            chg[0] = 0;
        }
        __syncthreads();  // B

        // the flood
        for (int it = 0; it < most; ++it) {
            bool changed = false;
            #pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = tid; i < nwords; i += nthreads) {
                const uint32_t rw = Rm[i], f = Fm[i];
                if ((rw & ~f) == 0) continue;  // nothing left to reach in this word
                const int y = i >> lgnw, k = i & (nw - 1);
                const int kp = (k - 1) & (nw - 1), kn = (k + 1) & (nw - 1);
                uint32_t m = 0, p = 0, n = 0;
                for (int d = -reach; d <= reach; ++d) {
                    // a row beyond a plane's border: the lane's own row once more, which changes nothing
                    const int yy = plane && (unsigned)(y + d) >= (unsigned)H ? y : (y + d) & (H - 1);
                    const uint32_t *row = Fm + (yy << lgnw);
                    m |= row[k];
                    p |= row[kp];
                    n |= row[kn];
                }
                if (plane) {  // no word beyond the border
                    p = k > 0 ? p : 0u;
                    n = k < nw - 1 ? n : 0u;
                } else if (width < 32) {
                    for (int s = width; s < 32; s <<= 1) m |= m << s;
                    p = n = m;
                }
                uint32_t g = m | __builtin_amdgcn_alignbit(m, p, 31) | __builtin_amdgcn_alignbit(n, m, 1);
                if (reach == 2) g |= __builtin_amdgcn_alignbit(m, p, 30) | __builtin_amdgcn_alignbit(n, m, 2);
                uint32_t nf = f | (g & rw);
                for (;;) {  // on inside the word: shifts within a word are neighbours on either topology
                    uint32_t t = (nf << 1) | (nf >> 1);
                    if (reach == 2) t |= (nf << 2) | (nf >> 2);
                    t = nf | (t & rw);
                    if (t == nf) break;
                    nf = t;
                }
                if (nf != f) {
                    Fm[i] = nf;
                    changed = true;
                }
            }
            const int slot = it % 3;
            if (changed) chg[slot] = 1;
            if (tid == 0) chg[slot == 2 ? 0 : slot + 1] = 0;
            __syncthreads();
            if (__builtin_amdgcn_readfirstlane((int)chg[slot]) == 0) break;  // one value for every wave
        }

        // pass 1
        {
            uint32_t pop = 0;
            cand = kObjNone;
            #pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = tid; i < nwords; i += nthreads) {
                const uint32_t f = Fm[i];
                uint32_t rw = Rm[i];
                if (f) {
                    const int y = i >> lgnw;
                    pop += (uint32_t)__builtin_popcount(f);
                    atomicOr(&st[kObjOccX + (i & (nw - 1))], f);
                    atomicOr(&st[kObjOccY + (y >> 5)], 1u << (y & 31));
                    rw &= ~f;
                    Rm[i] = rw;
                }
                if (rw && cand == kObjNone) cand = (uint32_t)i * 32u + (uint32_t)__builtin_ctz(rw);
            }
            pop = objects_wave_sum(pop);
            if (lane == 63 && pop) atomicAdd(&st[kObjPop], pop);
            cand = objects_wave_min(cand);
            if (lane == 63 && cand != kObjNone) atomicMin(&nx[kObjSeed], cand);
        }
        __syncthreads();  // C

        int x0 = 0, y0 = 0, w = 0, h = 0;
        uint32_t flags = 0;
        if (want) {
            if (objects_extent(st + kObjOccX, width, !plane, reach, x0, w)) flags |= kObjectWindsX;
            if (objects_extent(st + kObjOccY, H, !plane, reach, y0, h)) flags |= kObjectWindsY;
            uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
            bool any = false;
            #pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = tid; i < nwords; i += nthreads) {
                uint32_t f = Fm[i];
                if (!f) continue;
                any = true;
                const uint32_t dy = (uint32_t)(((i >> lgnw) - y0) & (H - 1)), ey = (uint32_t)(h - 1) - dy;
                const int xb = ((i & (nw - 1)) << 5) - x0;
                do {
                    const uint32_t dx = (uint32_t)((xb + __builtin_ctz(f)) & (width - 1)), ex = (uint32_t)(w - 1) - dx;
                    f &= f - 1;
                    s0 += objects_mix((uint64_t)(dy << 16 | dx));
                    s1 += objects_mix((uint64_t)(dy << 16 | ex));
                    s2 += objects_mix((uint64_t)(ey << 16 | dx));
                    s3 += objects_mix((uint64_t)(ey << 16 | ex));
                    s4 += objects_mix((uint64_t)(dx << 16 | dy));
                    s5 += objects_mix((uint64_t)(dx << 16 | ey));
                    s6 += objects_mix((uint64_t)(ex << 16 | dy));
                    s7 += objects_mix((uint64_t)(ex << 16 | ey));
                } while (f);
            }
            if (__builtin_amdgcn_ballot_w64(any) != 0) {  // per wave: DPP and LDS atomics inside, no barrier
                unsigned long long *sum = reinterpret_cast<unsigned long long *>(st + kObjSum);
                s0 = objects_wave_sum64(s0);
                s1 = objects_wave_sum64(s1);
                s2 = objects_wave_sum64(s2);
                s3 = objects_wave_sum64(s3);
                s4 = objects_wave_sum64(s4);
                s5 = objects_wave_sum64(s5);
                s6 = objects_wave_sum64(s6);
                s7 = objects_wave_sum64(s7);
                if (lane == 63) {
                    atomicAdd(&sum[0], (unsigned long long)s0);
                    atomicAdd(&sum[1], (unsigned long long)s1);
                    atomicAdd(&sum[2], (unsigned long long)s2);
                    atomicAdd(&sum[3], (unsigned long long)s3);
                    atomicAdd(&sum[4], (unsigned long long)s4);
                    atomicAdd(&sum[5], (unsigned long long)s5);
                    atomicAdd(&sum[6], (unsigned long long)s6);
                    atomicAdd(&sum[7], (unsigned long long)s7);
                }
            }
        }
        __syncthreads();  // D

        if (want && tid == 0) {
            const unsigned long long *sum = reinterpret_cast<const unsigned long long *>(st + kObjSum);
            const uint64_t box_wh = objects_mix((uint64_t)1 << 32 | (uint64_t)h << 16 | (uint64_t)w);
            const uint64_t box_hw = objects_mix((uint64_t)1 << 32 | (uint64_t)w << 16 | (uint64_t)h);
            uint64_t best = (uint64_t)sum[0] ^ box_wh;
            for (int k = 1; k < 8; ++k) {
                const uint64_t hk = (uint64_t)sum[k] ^ (k < 4 ? box_wh : box_hw);
                best = hk < best ? hk : best;
            }
            if (plane && (x0 == 0 || y0 == 0 || x0 + w == width || y0 + h == H)) flags |= kObjectAtBorder;
            ObjectRecord *rec = objects + ((int64_t)blockIdx.x * window + (count - first));
            rec->x = x0;
            rec->y = y0;
            rec->w = w;
            rec->h = h;
            rec->population = (int32_t)st[kObjPop];
            rec->flags = flags;
            rec->hash = best;
        }
    }
    if (tid == 0) nobjects[blockIdx.x] = count;
}

// Dynamic LDS of one workgroup: the sums, R and F.
inline size_t objects_lds_bytes(int width, int height) {
    const size_t nw = width >= 32 ? (size_t)width / 32 : 1;
    return sizeof(uint32_t) * ((size_t)kObjCtrl + 2 * nw * (size_t)height);
}

}  // namespace
}  // namespace golhip
