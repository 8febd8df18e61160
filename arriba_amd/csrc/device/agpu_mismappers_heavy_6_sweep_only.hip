// arriba_amd/csrc/device/agpu_mismappers_heavy_6_sweep_only.hip -- mismapper_heavy_kernel<6, true>: 6 wavefronts per SIMD, SWEEP_ONLY (the searches go through the sweep or are given up).
// A translation unit of its own: see mismapper_heavy.hpp.
#include "mismapper_heavy.hpp"

AGPU_MISMAPPER_HEAVY_LAUNCHER(launch_mismapper_heavy_6_sweep_only, 6, true)
