// eval_shared.hpp -- the device pieces the evaluator (eval.hip) and the query
// unit (predict.hip) both need: the filter-set probe, the per-relation
// projection kernel and the rank / score tile width.  One definition, included
// by both translation units (internal linkage in each).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "eval.hpp"
#include "hip_util.hpp"

namespace kb2e {
namespace {

constexpr int kQ = 16;  // queries per rank / score tile
constexpr size_t kLdsMax = 160 * 1024;

// host_data.hpp mix64 on the device: the FilterSet slot of a key
__device__ __forceinline__ uint64_t eval_mix64(uint64_t x) {
    x ^= x >> 31;
    x *= 0x7fb5d329728ea185ull;
    x ^= x >> 27;
    x *= 0x81dadef4bc2dd44dull;
    x ^= x >> 33;
    return x;
}

struct FilterView {
    const uint64_t* slots;
    uint64_t mask, nr64, ne64;
    __device__ __forceinline__ bool has(int64_t h, int64_t r, int64_t t) const {
        const uint64_t k = ((uint64_t)h * nr64 + (uint64_t)r) * ne64 + (uint64_t)t;
        uint64_t p = eval_mix64(k) & mask;
        while (true) {
            const uint64_t s = slots[p];
            if (s == k) return true;
            if (s == ~0ull) return false;
            p = (p + 1) & mask;
        }
    }
};

template <typename T>
struct ProjArgs {
    int32_t model, n, ld, ne, r;
    const T* ent;
    const T* rel;
    const T* w;
    double* PT;    // [n][ne]
    double* relv;  // [n] relation r in FP64
};

// One thread per entity: its projection for relation r, in FP64, summed in the
// reference's order.
template <typename T>
__global__ __launch_bounds__(256) void eval_project_kernel(ProjArgs<T> a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = i; k < a.n; k += (int)(gridDim.x * blockDim.x)) a.relv[k] = (double)a.rel[(int64_t)a.r * a.ld + k];
    if (i >= a.ne) return;
    const T* e = a.ent + (int64_t)i * a.ld;
    if (a.model == 0) {
        for (int k = 0; k < a.n; ++k) a.PT[(int64_t)k * a.ne + i] = (double)e[k];
    } else if (a.model == 1) {
        const T* w = a.w + (int64_t)a.r * a.ld;
        double s = 0;
        for (int k = 0; k < a.n; ++k) s += (double)w[k] * (double)e[k];
        for (int k = 0; k < a.n; ++k) a.PT[(int64_t)k * a.ne + i] = (double)e[k] - s * (double)w[k];
    } else {
        const T* W = a.w + (int64_t)a.r * a.n * a.ld;
        for (int k = 0; k < a.n; ++k) {
            double s = 0;
            for (int j = 0; j < a.n; ++j) s += (double)W[(int64_t)j * a.ld + k] * (double)e[j];
            a.PT[(int64_t)k * a.ne + i] = s;
        }
    }
}

template <typename K>
void allow_lds(K kernel, size_t bytes) {
    HIPCHK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

template <typename T>
void project(const EvalTables& t, int r, double* PT, double* relv) {
    ProjArgs<T> a{t.model, t.n, t.ld, t.ne, r, (const T*)t.ent, (const T*)t.rel, (const T*)t.w, PT, relv};
    eval_project_kernel<T><<<(std::max(t.ne, t.n) + 255) / 256, 256, 0, t.stream>>>(a);
    HIPCHK(hipGetLastError());
}

inline void project_any(const EvalTables& t, int r, double* PT, double* relv) {
    if (t.f64) project<double>(t, r, PT, relv);
    else project<float>(t, r, PT, relv);
}

}  // namespace
}  // namespace kb2e
