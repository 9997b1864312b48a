// Range probe: (max |x|, finite values with |x| > 65504, non-finite values) of a strided 2-D fp32 view, reduced on the device
// (range_probe.hip). The diagnostic behind the range report: how far a checkpoint's activations are from the limit of the
// split-f16 storage format (sf.h).
#pragma once
#include "common.h"

namespace atdn {

// one result slot in device memory; zero it (hipMemsetAsync) before the first launch that adds into it
struct RangeSlot {
  unsigned int max_bits;         // bit pattern of the largest finite |x| (non-negative floats order like their bit patterns)
  unsigned int pad_;
  unsigned long long over;       // finite values with |x| > 65504 (65504 itself is representable and not counted: sf.h)
  unsigned long long nonfinite;  // infinities and NaNs, by exponent bits; they do not enter the maximum
};
static_assert(sizeof(RangeSlot) == 24, "RangeSlot layout");

// x: `rows` rows of `cols` valid values, row pitch `ld` floats (ld >= cols unless rows <= 1); any 4-byte aligned address.
// Adds into *slot (maximum / sums). A pure read; nothing is launched for an empty view. Capturable: no allocation, no sync.
void launch_range_probe(const float* x, long rows, long cols, long ld, RangeSlot* slot, hipStream_t st);

}  // namespace atdn
