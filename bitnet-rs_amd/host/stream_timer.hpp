// stream_timer.hpp -- the host layer's one timed bracket: two events around a span of launches on one stream.
#pragma once

#include <hip/hip_runtime_api.h>

namespace bitnet_host {

// start() creates the two events and records the first; stop() records the second, SYNCHRONISES the stream and stores the span in
// *ms (nullable).  The events go with the object: an error return between the two must not leak them.
class StreamTimer {
  public:
    StreamTimer() = default;
    StreamTimer(const StreamTimer &) = delete;
    StreamTimer &operator=(const StreamTimer &) = delete;
    ~StreamTimer() {
        if (e0_) hipEventDestroy(e0_);
        if (e1_) hipEventDestroy(e1_);
    }
    hipError_t start(hipStream_t s) {
        hipError_t e = e0_ ? hipSuccess : hipEventCreate(&e0_);
        if (e == hipSuccess && !e1_) e = hipEventCreate(&e1_);
        return e == hipSuccess ? hipEventRecord(e0_, s) : e;
    }
    hipError_t stop(hipStream_t s, float *ms) {
        hipError_t e = hipEventRecord(e1_, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        float t = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0_, e1_);
        if (e == hipSuccess && ms) *ms = t;
        return e;
    }

  private:
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

}  // namespace bitnet_host
