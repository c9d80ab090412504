// binding_result.h -- who owns the buffer a call's result is written to.  No pybind11 here: tests/cxx/binding_result_check.cpp builds this file alone,
// with a memory policy that counts.
#pragma once

#include <cstddef>

namespace gbrl_py {

// `count` elements on device `device_id` (Mem::alloc; null when that fails) or new[] on the host -- or the caller's own buffer, adopted: get() returns
// it and nothing is ever freed.  An owned buffer is freed by the destructor unless take() has handed it on.
template <typename T, typename Mem>
class ResultBuffer {
   public:
    ResultBuffer(bool on_device, int device_id, size_t count) : dev_(on_device), dev_id_(on_device ? device_id : 0) {
        if (dev_) p_ = static_cast<T *>(Mem::alloc(dev_id_, sizeof(T) * count));
        else p_ = new T[count];
    }
    struct Adopt {};
    ResultBuffer(Adopt, T *callers, bool on_device) : p_(callers), dev_(on_device), adopted_(true) {}
    ResultBuffer(const ResultBuffer &) = delete;
    ResultBuffer &operator=(const ResultBuffer &) = delete;
    ~ResultBuffer() {   // still owned: the call has failed
        if (!p_ || adopted_) return;
        if (dev_) Mem::free(p_); else delete[] p_;
    }
    T *get() const { return p_; }
    bool on_device() const { return dev_; }
    int device_id() const { return dev_id_; }
    bool adopted() const { return adopted_; }
    T *take() {   // the buffer is the caller's from here on
        T *p = p_;
        p_ = nullptr;
        return p;
    }

   private:
    T *p_ = nullptr;
    bool dev_;
    int dev_id_ = 0;
    bool adopted_ = false;
};

}  // namespace gbrl_py
