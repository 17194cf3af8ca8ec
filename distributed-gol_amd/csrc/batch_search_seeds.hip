// batch_search_seeds.hip -- gol_batch_search constant-folded for Seeds (B2/S): every board shape.
#include "batch_search.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_SEARCH_CONST(0x004, 0x000)
}  // namespace golhip
