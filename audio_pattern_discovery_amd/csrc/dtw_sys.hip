// Instantiates the systolic fused-pair DTW kernels for frame dimension APD_DIM (the Makefile compiles this unit once per D:
// parallel builds, per-family compiler flags).
#include "dtw_systolic.h"
namespace apd {
template decltype(launch_systolic<APD_DIM>) launch_systolic<APD_DIM>;
}
