// batch_plane_box.hip -- batch_clip_box: the soup box of golhip_batch_init_random.  The boxed soup of a
// seed is the full-board soup with every cell outside the box cleared, so the box is one AND per
// word over the boards batch_init_random (batch_board.hip, untouched) has just written, with the
// mask gol_plane_search applies to the words it seeds (box_word_mask, golhip_internal.hpp).
#include <algorithm>

#include "golhip_internal.hpp"

namespace golhip {
namespace {

__global__ void batch_clip_box(uint32_t *__restrict__ boards, int64_t board_pitch, int64_t nboards, int64_t rows,
                               int32_t width, int32_t wd, SoupBox box) {
    const int64_t per = rows * wd, n = nboards * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bi = i / per, ib = i - bi * per;
        const int64_t y = ib / wd;
        const int32_t col = (int32_t)(ib - y * wd);
        boards[bi * board_pitch + ib] &= box_word_mask(y, col, width, box);
    }
}

}  // namespace

hipError_t launch_batch_clip_box(uint32_t *boards, int64_t board_pitch, int64_t nboards, int64_t rows, int64_t width,
                                 int32_t wd, const SoupBox &box, hipStream_t s) {
    if (nboards < 1 || rows < 1 || width < 32 || width % 32 != 0 || width > 32 * (int64_t)wd ||
        board_pitch < rows * wd || box.w < 1 || box.h < 1 || box.x0 < 0 || box.y0 < 0 || box.x0 + box.w > width ||
        box.y0 + box.h > rows)
        return hipErrorInvalidValue;
    const int64_t n = nboards * rows * wd;
    const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 1 << 16);
    hipLaunchKernelGGL(batch_clip_box, dim3(grid), dim3(256), 0, s, boards, board_pitch, nboards, rows, (int32_t)width,
                       wd, box);
    return hipGetLastError();
}

}  // namespace golhip
