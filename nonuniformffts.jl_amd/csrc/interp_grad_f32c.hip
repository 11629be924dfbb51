// gradient gather, T = float, complex = true (see interp_grad_kernels.h).
#define NUFFT_T float
#define NUFFT_CPLX true
#define NUFFT_GRAD_LAUNCHER launch_interp_grad_f32c
#include "interp_grad_inst.h"
