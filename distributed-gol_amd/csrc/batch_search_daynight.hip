// batch_search_daynight.hip -- gol_batch_search constant-folded for Day & Night (B3678/S34678): every board shape.
#include "batch_search.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_SEARCH_CONST(0x1C8, 0x1D8)
}  // namespace golhip
