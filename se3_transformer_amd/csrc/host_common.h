// Host-side launch helpers shared by every .hip file; no device code.
#pragma once

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/HIPContext.h>

// Closes an entry point: a failed launch raises, prefixed by `what`.
static inline void check_launch(const char* what) {
    hipError_t err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, what, hipGetErrorString(err));
}

// x's storage as T*, also for the bf16 types data_ptr<T>() does not know.
template <class T>
static inline T* tptr(const torch::Tensor& x) {
    return reinterpret_cast<T*>(x.data_ptr());
}

// Body with T = float for an fp32 x, T = BF16 (the file's bf16 type) for a
// bf16 one; any other dtype is an error.
#define DISPATCH_F32_BF16(x, BF16, ...)                                \
    if ((x).dtype() == torch::kFloat32) {                              \
        using T = float; __VA_ARGS__;                                  \
    } else {                                                           \
        TORCH_CHECK((x).dtype() == torch::kBFloat16);                  \
        using T = BF16; __VA_ARGS__;                                   \
    }

// Body with constexpr int K = V for an order V = 2d+1 in {1, 3, 5, 7}.
#define DISPATCH_ORDER(V, K, what, ...)                                \
    switch (V) {                                                       \
        case 1: { constexpr int K = 1; __VA_ARGS__; break; }           \
        case 3: { constexpr int K = 3; __VA_ARGS__; break; }           \
        case 5: { constexpr int K = 5; __VA_ARGS__; break; }           \
        case 7: { constexpr int K = 7; __VA_ARGS__; break; }           \
        default: TORCH_CHECK(false, "unsupported " what " ", V);       \
    }
