// batch_search_highlife.hip -- gol_batch_search constant-folded for HighLife (B36/S23): every board shape.
#include "batch_search.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_SEARCH_CONST(0x048, 0x00C)
}  // namespace golhip
