// batch_objects.hip -- gol_batch_objects (batch_objects.hpp), the kernel of golhip_batch_objects and
// golhip_batch_search_objects, and its launcher: one translation unit, one kernel.  The launcher sizes
// the workgroup and its dynamic LDS from the shape: a lane per word of the board up to 1024 lanes,
// the two bitmaps of that board size, so small boards keep many workgroups on a CU and a 512 x 512
// board takes one (64.4 KiB).
#include <algorithm>

#include "batch_objects.hpp"

namespace golhip {

hipError_t launch_batch_objects(int nboards, const BatchObjectsParams &op, hipStream_t s) {
    const int32_t w = op.width, h = op.height;
    // the shapes golhip_batch_create makes: powers of two, a row of the torus in wd words
    if (nboards < 1 || nboards > 65536 || !op.boards || !op.nobjects || (op.reach != 1 && op.reach != 2) ||
        op.max_objects < 1 || op.max_objects > kObjectsMax || op.first < 0 || op.window < 1 || w < 1 || w > 512 ||
        (w & (w - 1)) != 0 || h < 4 || h > 512 || (h & (h - 1)) != 0 || (op.wd != 4 && op.wd != 8 && op.wd != 16) ||
        w > 32 * op.wd || op.board_pitch < (int64_t)h * op.wd)
        return hipErrorInvalidValue;
    const int nwords = (w >= 32 ? w / 32 : 1) * h;
    const int threads = std::min(1024, (nwords + 63) / 64 * 64);
    const size_t lds = objects_lds_bytes(w, h);
    if (lds > 64 * 1024) {  // beyond the default limit of a launch: gfx950 gives a workgroup up to 160 KiB
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(gol_batch_objects),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gol_batch_objects, dim3((unsigned)nboards), dim3((unsigned)threads), lds, s, op.boards,
                       op.board_pitch, op.wd, w, h, op.plane ? 1 : 0, op.reach, op.max_objects, op.first, op.window,
                       op.nobjects, op.objects);
    return hipGetLastError();
}

}  // namespace golhip
