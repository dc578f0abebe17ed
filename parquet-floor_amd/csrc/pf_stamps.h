// pf_stamps.h — phase-stamp tables of -DPF_STAMPS builds (in-kernel s_memtime sums, read by tools/probe_*.py).
//
// PF_STAMP_TABLE(table, N, reader) defines `__device__ unsigned long long table[N]` and its host reader
// `extern "C" int reader(unsigned long long* out, int n, int reset)`, which copies the first min(n, N) slots to
// out and then, if reset, zeroes the table (0, or -1 on a HIP error). A __device__ array belongs to one unit (no
// relocatable device code): each table has one use of the macro, and only that unit's kernels stamp into it.
#pragma once

#define PF_STAMP_TABLE(table, N, reader)                                                                          \
    __device__ unsigned long long table[N];                                                                       \
    extern "C" int reader(unsigned long long* out, int n, int reset) {                                            \
        if (hipMemcpyFromSymbol(out, HIP_SYMBOL(table), sizeof(unsigned long long) * (n < (N) ? n : (N))) != hipSuccess) return -1; \
        if (reset) {                                                                                              \
            unsigned long long z[N] = {};                                                                         \
            if (hipMemcpyToSymbol(HIP_SYMBOL(table), z, sizeof z) != hipSuccess) return -1;                       \
        }                                                                                                         \
        return 0;                                                                                                 \
    }
