// lsn_hip.h - what every host file that talks to the HIP runtime shares: the one HIP_CHECK, the one clock and the one entry guard.
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

}  // namespace lsn

#define HIP_CHECK(x) ::lsn::hip_check((x), #x)
