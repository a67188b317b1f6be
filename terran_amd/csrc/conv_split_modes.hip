// The split-role kernels (conv_split_kernels.h) in the modes f32, bf16x3, bf16 and f16; called by ta_launch_conv_split
// (conv_split.hip), which also runs the second pass of a K-split launch.
#include "conv_split_kernels.h"

TA_TRACE_READER(ta_debug_trace_read_split_modes)

int ta_launch_conv_split_modes(ta_ctx* ctx, int v, const ta_conv_launch& p) {
  switch (p.prec) {
    case PREC_F32: return launch_split_variant<PREC_F32>(ctx, v, p);
    case PREC_BF16X3: return launch_split_variant<PREC_BF16X3>(ctx, v, p);
    case PREC_F16: return launch_split_variant<PREC_F16>(ctx, v, p);
    default: return launch_split_variant<PREC_BF16>(ctx, v, p);
  }
}
