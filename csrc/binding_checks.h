// Argument checks shared by the torch extension bindings
// (csrc/gpu_bindings.cpp, csrc/gpu_ctl_bindings.cpp): the native boundary,
// the only place where a Python tensor becomes a raw pointer.  Every op is an
// `Op` (the checks), a list of (tensor, element type, length) reads through
// Op::ptr, and one launch.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip/dataplane.h"

// The torch element type that stores a kernel-side T: the kernels read int64
// storage as u64 words and int32 storage as u32 words or as PairRec rows.
template <typename T> struct Stored { using type = T; };
template <> struct Stored<uint64_t> { using type = int64_t; };
template <> struct Stored<uint32_t> { using type = int32_t; };
template <> struct Stored<PairRec> { using type = int32_t; };  // [cap][4], see Op::pairs

// The shape an op states for an argument; -1 leaves a field open.
struct Shape { int64_t dim = -1, rows = -1, cols = -1; };
static constexpr Shape vec() { return {1, -1, -1}; }
static constexpr Shape mat(int64_t rows = -1, int64_t cols = -1) { return {2, rows, cols}; }

// One op's argument checks.  ptr() vets a tensor (dtype, stated shape,
// contiguity, minimum length) and hands out its pointer; i32() narrows a
// size or scalar.  Neither needs a GPU.  begin() then makes the device checks
// for every tensor seen so far, in argument order, so a machine without a GPU
// still exercises everything before them, and switches to the first tensor's
// device for the rest of the op.  launched() looks at the launch result.
// The tensors passed to ptr() must outlive the Op (they are the op's named
// arguments and locals, never temporaries).
class Op {
public:
    enum Where { kDevice, kPinnedHost };

    explicit Op(const char* name) : name_(name) {}

    template <typename T>
    T* ptr(const torch::Tensor& t, const char* arg, int64_t min_numel = 0, Shape shape = {},
           Where where = kDevice) {
        using S = typename Stored<T>::type;
        constexpr auto want = c10::CppTypeToScalarType<S>::value;
        TORCH_CHECK(t.scalar_type() == want, name_, ": ", arg, " must be ", c10::toString(want),
                    ", got ", c10::toString(t.scalar_type()));
        TORCH_CHECK(shape.dim < 0 || t.dim() == shape.dim, name_, ": ", arg, " must have ",
                    shape.dim, " dimension(s), got sizes ", t.sizes());
        TORCH_CHECK((shape.rows < 0 || t.size(0) == shape.rows)
                    && (shape.cols < 0 || t.size(1) == shape.cols),
                    name_, ": ", arg, " must be [", shape.rows, ", ", shape.cols,
                    "] (-1: any), got sizes ", t.sizes());
        TORCH_CHECK(t.is_contiguous(), name_, ": ", arg, " must be contiguous, got sizes ",
                    t.sizes(), " with strides ", t.strides());
        TORCH_CHECK(t.numel() >= min_numel, name_, ": ", arg, " needs at least ", min_numel,
                    " elements, got ", t.numel());
        TORCH_CHECK(n_seen_ < kMaxSeen, name_, ": too many tensor arguments");
        seen_[n_seen_++] = {arg, &t, where};
        return reinterpret_cast<T*>(t.data_ptr<S>());
    }

    // ptr() for an argument that has exactly n elements; `per` says which
    // argument's length sets n ("one per disc").
    template <typename T>
    T* same(const torch::Tensor& t, const char* arg, int64_t n, const char* per,
            Shape shape = {}) {
        T* p = ptr<T>(t, arg, n, shape);
        TORCH_CHECK(t.numel() == n, name_, ": ", arg, " must have exactly ", n, " elements (",
                    per, "), got ", t.numel());
        return p;
    }

    PairRec* pairs(const torch::Tensor& t, const char* arg = "pairs") {
        return ptr<PairRec>(t, arg, 0, mat(-1, 4));
    }

    // The one narrowing of a size or scalar to 32 bits.
    int32_t i32(int64_t v, const char* what, int64_t lo = 0, int64_t hi = INT32_MAX) const {
        TORCH_CHECK(v >= lo && v <= hi, name_, ": ", what, " = ", v, " is outside [", lo, ", ",
                    hi, "]");
        return (int32_t)v;
    }

    void ring_bytes(int64_t v) const {
        TORCH_CHECK(v >= 0 && v % 16 == 0, name_, ": ring_bytes = ", v,
                    " must be a non-negative multiple of 16");
    }

    // Device checks, last on purpose; returns the stream to launch on.
    hipStream_t begin() {
        TORCH_CHECK(n_seen_ > 0, name_, ": no tensor argument");
        const c10::Device dev = seen_[0].t->device();
        for (int i = 0; i < n_seen_; ++i) {
            const torch::Tensor& t = *seen_[i].t;
            if (seen_[i].where == kPinnedHost) {
                TORCH_CHECK(!t.is_cuda() && t.is_pinned(), name_, ": ", seen_[i].arg,
                            " must be a pinned CPU tensor, got one on ", t.device());
                continue;
            }
            TORCH_CHECK(t.is_cuda(), name_, ": ", seen_[i].arg, " must be on a GPU, got ",
                        t.device());
            TORCH_CHECK(t.device() == dev, name_, ": ", seen_[i].arg, " is on ", t.device(),
                        " but ", seen_[0].arg, " is on ", dev);
        }
        guard_.reset_device(dev);
        return at::hip::getCurrentHIPStream().stream();
    }

    // After each launcher call.  Reads the launch error only: no
    // synchronisation, so it is safe under stream capture.
    void launched() const { check(hipGetLastError(), "kernel launch"); }

    void check(hipError_t e, const char* what) const {
        TORCH_CHECK(e == hipSuccess, name_, ": ", what, " failed: ", hipGetErrorString(e));
    }

    const char* name() const { return name_; }

private:
    struct Seen { const char* arg; const torch::Tensor* t; Where where; };
    static constexpr int kMaxSeen = 16;
    const char* name_;
    Seen seen_[kMaxSeen];
    int n_seen_ = 0;
    c10::OptionalDeviceGuard guard_;
};

// Options for a new tensor of `dtype` on the device of `like`.
static inline torch::TensorOptions opts(torch::ScalarType dtype, const torch::Tensor& like) {
    return torch::TensorOptions().dtype(dtype).device(like.device());
}
