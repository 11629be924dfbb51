// gradient gather, T = double, complex = true (see interp_grad_kernels.h).
#define NUFFT_T double
#define NUFFT_CPLX true
#define NUFFT_GRAD_LAUNCHER launch_interp_grad_f64c
#include "interp_grad_inst.h"
