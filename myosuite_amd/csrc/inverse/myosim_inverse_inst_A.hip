// explicit instantiations of k_inverse: the 4-wide limit-row kernels and the 24-wide general-row kernel (Euler entries of the engine list, myosim_inst_list.hpp)
#include "myosim_inverse_kernel.hpp"
MM_KERNELS_A(MMI_INSTANTIATE) MM_KERNELS_I(MMI_INSTANTIATE)
