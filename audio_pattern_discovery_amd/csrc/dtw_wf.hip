// Instantiates the wide-band and full-matrix fused-pair DTW kernels for frame dimension APD_DIM (one unit per D, see the Makefile).
#include "dtw_wide.h"
#include "dtw_full.h"
namespace apd {
template decltype(launch_wide<APD_DIM>) launch_wide<APD_DIM>;
template decltype(launch_full<APD_DIM>) launch_full<APD_DIM>;
}
