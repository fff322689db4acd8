// Error reporting of libdq_hip.so, free of HIP: what a host-only translation unit (dq_sampler_tables.cpp) shares with the rest through dq_common.h.
#pragma once
#include <string>

namespace dq {

void set_error(const std::string& msg);  // the calling thread's dq_last_error() (dq_api.hip)

#define DQ_REQUIRE(cond, msg)                                                                      \
  do {                                                                                             \
    if (!(cond)) {                                                                                 \
      dq::set_error(std::string(msg) + " [" #cond "] (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
      return 2;                                                                                    \
    }                                                                                              \
  } while (0)

}  // namespace dq
