// explicit instantiations of k_inverse: the 36-wide general-row kernel (leg models) (Euler entries of the engine list, myosim_inst_list.hpp)
#include "myosim_inverse_kernel.hpp"
MM_KERNELS_H(MMI_INSTANTIATE)
