// frp_capi_internal.hpp -- what the three units of the C-ABI share: frp_capi.hip defines it, frp_dropin.hip and frp_host_batch.hip use it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include "../../include/frp_nmpc.h"
#include "frp_kernels.h"

#define FRP_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "[frp_nmpc] HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            return FRP_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)

namespace frp::capi {
// shape, model and the arrays every solve needs: the one check of a frp_nmpc_batch, before anything is sized or copied from its pointers
bool batch_shape_ok(const frp_nmpc_batch *b);
// frp_nmpc_options.timeout -> KernelArgs::deadline (ticks of the wall clock, rounded up; 0 = no budget) / timeout_invalid.  False only
// when a budget is set and the clock's rate cannot be read (no device).
bool budget_args(double timeout, frp::KernelArgs *a);
bool fill_args(const frp_nmpc_batch *b, const frp_nmpc_options *opt_in, void *ws, size_t ws_bytes, frp::KernelArgs *a);
} // namespace frp::capi
