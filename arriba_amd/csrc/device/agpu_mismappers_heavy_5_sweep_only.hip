// arriba_amd/csrc/device/agpu_mismappers_heavy_5_sweep_only.hip -- mismapper_heavy_kernel<5, true>: 5 wavefronts per SIMD, SWEEP_ONLY (the searches go through the sweep or are given up).
// A translation unit of its own: see mismapper_heavy.hpp.
#include "mismapper_heavy.hpp"

AGPU_MISMAPPER_HEAVY_LAUNCHER(launch_mismapper_heavy_5_sweep_only, 5, true)
