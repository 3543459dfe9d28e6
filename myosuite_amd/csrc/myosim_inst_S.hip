// explicit instantiations, group S: the two-rows-per-lane general-row kernels (see myosim_inst_list.hpp)
#include "myosim_engine_kernel.hpp"
#include "myosim_inst_list.hpp"
MM_KERNELS_S(MM_INSTANTIATE_ROWS2)
