// ps_coarse_band.h -- the block half-bandwidth of the folded path's coarse matrix A_c = P^T S^ P, from the run tables that
// k_coarse_rowsums / k_coarse_matrix sum over.  No HIP: tests/test_coarse_band_host.py compiles it with a plain C++ compiler
// and holds it against a numpy restatement.
//   block (q, q') of A_c is structurally non-zero  iff  some fine row i of supp(q) = [slo[q], shi[q]) has a non-empty run for q'
//   (run_lo[i ncb + q'] < run_hi[i ncb + q']): k_coarse_matrix starts the entry at 0.0 and adds w(i, q) SZ[i][q'] over exactly
//   those rows, SZ[i][q'] being a sum over exactly that run -- every other entry stays +0.0.
// -> max |q - q'| over the structural blocks; 0 for a single node, for empty supports and for rows without runs.  The caller
// hands k_coarse_chol_band this number (ncb - 1 is the dense matrix: a long loop closure gives that).
#pragma once
#include <cstdint>
#include <cstdlib>

inline int ps_coarse_band(int ncb, const int32_t* slo, const int32_t* shi, const int32_t* run_lo, const int32_t* run_hi)
{
    int bw = 0;
    for (int q = 0; q < ncb; ++q)
        for (int i = slo[q]; i < shi[q]; ++i)
            for (int q2 = 0; q2 < ncb; ++q2)
                if (run_hi[(size_t)i * ncb + q2] > run_lo[(size_t)i * ncb + q2] && std::abs(q - q2) > bw) bw = std::abs(q - q2);
    return bw;
}
