// lsn_hip.h - what every host file that talks to the HIP runtime shares: the one HIP_CHECK, the one clock, the one entry guard, and the scope guards of a
// stream and of a device allocation.
#pragma once
#include "../../../include/ltesniffer_amd.h"
#include "lsn_types.h"
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <string>

static_assert(LSN_FMT_CF32 == LSN_FILE_CF32 && LSN_FMT_SC16 == LSN_FILE_SC16 && LSN_FMT_SC8 == LSN_FILE_SC8, "lsn_sample_format speaks the public header's formats");

namespace lsn {

inline void hip_check(hipError_t e, const char* what)
{
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e) + " at " + what);
}

inline double now_ms()
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// adds the milliseconds its scope took to acc
struct ScopeTimer {
  explicit ScopeTimer(double& a) : t0(now_ms()), acc(a) {}
  ~ScopeTimer() { acc += now_ms() - t0; }
  const double t0;
  double& acc;
};

// entry guard of the calls that report through a return code: an exception on the way becomes one line on stderr and LSN_ERROR
template <class F>
int guarded(F&& f)
{
  try {
    return f();
  } catch (const std::exception& ex) {
    fprintf(stderr, "ltesniffer_amd: %s\n", ex.what());
    return LSN_ERROR;
  }
}

// the stand-alone entry points' test in front of their first allocation (the engine's own check, lsn_engine.cc / lsn_capi.cc, asks a different question)
inline bool have_device(int device)
{
  int ndev = 0;
  return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && device >= 0 && device < ndev;
}

// a stream of the current device, destroyed with its scope
struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() { hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreateWithFlags"); }
  ~OwnedStream() { (void)hipStreamDestroy(s); }
  OwnedStream(const OwnedStream&) = delete;
  OwnedStream& operator=(const OwnedStream&) = delete;
  operator hipStream_t() const { return s; }
};

// one device allocation, freed with its scope
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  template <typename T> T* alloc(size_t n) { hip_check(hipMalloc(&p, (n ? n : 1) * sizeof(T)), "hipMalloc"); return (T*)p; }
};

}  // namespace lsn

#define HIP_CHECK(x) ::lsn::hip_check((x), #x)
