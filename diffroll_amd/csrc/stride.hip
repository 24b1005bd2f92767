// gfx950 (MI355X, CDNA4): option "guidance_stride" - the guidance update computed at every n-th guided step and reused in
// between (the CFG cache of FasterCache, Lv et al. 2024; "Adaptive Guidance", Castillo et al. 2023).  A guided step under the
// option runs, behind the head projections, update_stride_kernel - a further instantiation of update_quad:
//   a step that refreshes   both evaluations ran; d = y - c stored over the engine's state, y consumed unchanged;
//   a step that reuses      the conditional evaluation alone ran; y = c + d consumed.
// The element's own thread is the only reader and writer of its word of the state; nothing waits, nothing is atomic, and
// refresh / reuse is a kernel argument baked per node: a captured chain replays with no host help, and its first guided
// step, a refresh, overwrites whatever the state held.
#include "stride_quad.h"

namespace dr {
#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void update_stride_kernel(const UpdateArgs a, const StrideUpd su) {
    const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
    if (i4 * 4 >= a.n) return;
    float4 y;
    reinterpret_cast<float4*>(a.x)[i4] = update_quad(a, i4, &y, su);
    if (a.mode == 5 && hist_next(a)) reinterpret_cast<float4*>(hist_next(a))[i4] = y;
}

hipError_t launch_update_stride(const UpdateArgs& a, const StrideUpd& su, hipStream_t s) {
    if (!su.d || !a.x0c || a.n % 4 || (su.reuse ? a.x0u != nullptr : a.x0u == nullptr)) return hipErrorInvalidValue;
    const long n4 = a.n / 4;
    hipLaunchKernelGGL(update_stride_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a, su);
    return hipGetLastError();
}

}  // namespace dr
