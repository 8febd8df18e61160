// arriba_amd/csrc/device/agpu_mismappers_heavy_4_everything.hip -- mismapper_heavy_kernel<4, false>: 4 wavefronts per SIMD, the kernel that holds everything (sweep, task lists and the recursion).
// A translation unit of its own: see mismapper_heavy.hpp.
#include "mismapper_heavy.hpp"

AGPU_MISMAPPER_HEAVY_LAUNCHER(launch_mismapper_heavy_4_everything, 4, false)
