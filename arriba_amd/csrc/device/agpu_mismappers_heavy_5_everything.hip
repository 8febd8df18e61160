// arriba_amd/csrc/device/agpu_mismappers_heavy_5_everything.hip -- mismapper_heavy_kernel<5, false>: 5 wavefronts per SIMD, the kernel that holds everything (sweep, task lists and the recursion).
// A translation unit of its own: see mismapper_heavy.hpp.
#include "mismapper_heavy.hpp"

AGPU_MISMAPPER_HEAVY_LAUNCHER(launch_mismapper_heavy_5_everything, 5, false)
