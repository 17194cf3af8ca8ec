// batch_census.hip -- gol_batch_census (batch_census.hpp), the kernel of golhip_batch_census, and its
// launcher: one translation unit, one kernel.  The launcher sizes the workgroup and its dynamic LDS
// from the shape: a lane per 32 anchors up to 1024 lanes, the frame (and the cover, with a residue
// output) of that board size, so small boards keep many workgroups on a CU and a 512 x 512 board
// takes one (83 KB with the cover).
#include <algorithm>

#include "batch_census.hpp"

namespace golhip {

hipError_t launch_batch_census(int nboards, const BatchCensusParams &cp, hipStream_t s) {
    const int32_t w = cp.width, h = cp.height;
    // the shapes golhip_batch_create makes: powers of two, a row of the torus in wd words
    if (nboards < 1 || nboards > 65536 || !cp.boards || !cp.patterns || cp.npat < 1 || cp.npat > kCensusMaxPatterns ||
        (!cp.counts && !cp.residue) || w < 1 || w > 512 || (w & (w - 1)) != 0 || h < 4 || h > 512 ||
        (h & (h - 1)) != 0 || (cp.wd != 4 && cp.wd != 8 && cp.wd != 16) || w > 32 * cp.wd ||
        cp.board_pitch < (int64_t)h * cp.wd)
        return hipErrorInvalidValue;
    const int nw = w >= 32 ? w / 32 : 1;
    const int items = cp.plane ? (h + kCensusMargin) * (nw + 1) : h * nw;
    const int threads = std::min(1024, (items + 63) / 64 * 64);
    const size_t lds = census_lds_bytes(w, h, cp.npat, cp.residue != nullptr);
    if (lds > 64 * 1024) {  // beyond the default limit of a launch: gfx950 gives a workgroup up to 160 KiB
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(gol_batch_census),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gol_batch_census, dim3((unsigned)nboards), dim3((unsigned)threads), lds, s, cp.boards,
                       cp.board_pitch, cp.wd, w, h, cp.plane ? 1 : 0, cp.patterns, cp.npat, cp.counts, cp.residue);
    return hipGetLastError();
}

}  // namespace golhip
