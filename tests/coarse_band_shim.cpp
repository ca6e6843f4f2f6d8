// C entry to csrc/ps_coarse_band.h for tests/test_coarse_band_host.py (plain C++ compiler, no HIP).
#include "ps_coarse_band.h"

extern "C" int coarse_band(int ncb, const int32_t* slo, const int32_t* shi, const int32_t* run_lo, const int32_t* run_hi) {
    return ps_coarse_band(ncb, slo, shi, run_lo, run_hi);
}
