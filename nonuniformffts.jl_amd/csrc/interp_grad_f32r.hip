// gradient gather, T = float, complex = false (see interp_grad_kernels.h).
#define NUFFT_T float
#define NUFFT_CPLX false
#define NUFFT_GRAD_LAUNCHER launch_interp_grad_f32r
#include "interp_grad_inst.h"
