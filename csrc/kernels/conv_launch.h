// The four conv launchers behind conv2d() (conv_mfma.hip), one per kernel. Each fills its args
// struct from the desc and its plan (gale/conv_route.h), picks the instantiation from the plan's
// fields and launches: no check, no geometry arithmetic, no global state. res is null unless the
// route was made with has_res.
#pragma once
#include "gale/kernels.h"

namespace gale {

hipError_t launch_conv_f32(const ConvDesc& d, const ConvF32Plan& p, const void* x, const void* w,
                           const float* bias, const void* res, void* y, hipStream_t stream);
hipError_t launch_conv_gemm(const ConvDesc& d, const ConvGemmPlan& p, const void* x,
                            const void* w, const float* bias, const void* res, void* y,
                            hipStream_t stream);
hipError_t launch_conv_patch(const ConvDesc& d, const ConvPatchPlan& p, const void* x,
                             const void* w, const float* bias, const void* res, void* y,
                             hipStream_t stream);
hipError_t launch_conv_mfma(const ConvDesc& d, const ConvMfmaPlan& p, const void* x,
                            const void* w, const float* bias, const float* wscale,
                            const void* res, void* y, hipStream_t stream);

}  // namespace gale
