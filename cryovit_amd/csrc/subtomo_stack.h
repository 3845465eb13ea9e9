// What the entries of subtomo.hip and align.hip refuse about a stack of boxes before they look at anything else.
#pragma once
#include "bit_rows.h"

namespace cvx {

// what is wrong with P and the box, or nullptr.  n = the voxels of a box
inline const char* stack_fault(long P, int box, long& n) {
    if (P < 0) return "P < 0";
    if (box < CVX_SUBTOMO_BOX_MIN || box > CVX_SUBTOMO_BOX_MAX || box % 2) return "box must be even and lie in [8, 128]";
    n = (long)box * box * box;
    if (P > CVX_SUBTOMO_MAX_PARTICLES) return "P must be <= 2^20";
    return nullptr;
}

}  // namespace cvx
