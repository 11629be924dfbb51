// gradient gather, T = double, complex = false (see interp_grad_kernels.h).
#define NUFFT_T double
#define NUFFT_CPLX false
#define NUFFT_GRAD_LAUNCHER launch_interp_grad_f64r
#include "interp_grad_inst.h"
