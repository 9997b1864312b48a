#include "conv_sf_dispatch_impl.h"
namespace atdn {
// (a unit of its own: with the 1x5 / 5x1 halo-patch shapes this epilogue is as much to compile as the other two of unit a together)
ATDN_INSTANTIATE_CONV_SF(SfBias<ACT_NONE>)
}
