// wavenet_wide_f32_gated_kernels.hip -- the gated instantiations of the exact-f32 kernel of the runtime-shaped family,
// WaveNetWideF32Kernel<2, true> and <4, true>: models with gated layer arrays (the A1 key "gated": z = act(filter half) * sigmoid(gate half))
// and some dimension above 16 channels, up to 64 everywhere, loaded on request (NA_SetWaveNetWideGated).  The code is
// wavenet_wide_f32_kernels.hip's (its header has the design), compiled a second time for these instantiations alone: a translation unit of
// its own, so that the plain instantiations come out of the compiler exactly as they did before (profiles/wide_gated_isa.txt).  Built with
// that file's flags: no contraction, no compiler-made packed f32.
#define NA_WIDE_F32_GATED_TU 1
#include "wavenet_wide_f32_kernels.hip"
