// The one formatter behind every refusal of the host layer: printf into 512 bytes, the text becomes the calling thread's
// misti_last_error, the code is returned.  Depends on misti_set_error_ alone (misti_api.cpp; the stand-ins of tests/multi_host define
// it for the host-only builds of misti_multi.cpp and misti_lanes.cpp).  Internal: never installed.
#pragma once
#include <cstdarg>
#include <cstdio>

extern "C" int misti_set_error_(int code, const char* msg);

namespace misti_host __attribute__((visibility("hidden"))) {

inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return misti_set_error_(code, buf);
}

}  // namespace misti_host
