// The CSR tap lists of the host's AREA tables (adaptiveisp_amd/resize.py: ptr[n + 1], idx[nnz], weight[nnz], 32-bit words,
// floats by their bits), as adaisp_resize_u8 (isp_resize.hip) and adaisp_raw_load (isp_raw_load.hip) read them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adaisp {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// one CSR tap list of an AREA table: row `k` of `n` rows at word `base` of `tabs` (checked to fit by the caller)
struct Csr {
    const int32_t* idx;
    const float* wt;
    int lo, hi;
};

__device__ __forceinline__ Csr csr_row(const int32_t* __restrict__ tab, int n, int k) {
    const int nnz = tab[n];
    Csr r;
    r.idx = tab + n + 1;
    r.wt = reinterpret_cast<const float*>(tab + n + 1 + nnz);
    r.lo = clampi(tab[k], 0, nnz);
    r.hi = clampi(tab[k + 1], r.lo, nnz);
    return r;
}

// an AREA table of n rows at word `base` lies inside tab_words (its nnz read only once the pointer array is known to fit)
__device__ __forceinline__ bool csr_fits(const int32_t* __restrict__ tabs, int64_t base, int n, int64_t tab_words) {
    if (base < 0 || base + n + 1 > tab_words) return false;
    const int64_t nnz = tabs[base + n];
    return nnz >= 0 && base + n + 1 + 2 * nnz <= tab_words;
}

}  // namespace adaisp
