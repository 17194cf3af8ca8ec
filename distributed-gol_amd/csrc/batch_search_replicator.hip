// batch_search_replicator.hip -- gol_batch_search constant-folded for Replicator (B1357/S1357): every board shape.
#include "batch_search.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_SEARCH_CONST(0x0AA, 0x0AA)
}  // namespace golhip
