// error.cpp -- the ldso_ba_last_error() message of each thread.  Host-only, so that the host-side
// pieces (layout.cpp) link into a CPU program without the device translation units.
#include "ldso_ba_internal.h"

namespace ldso_ba {

namespace {
thread_local std::string g_err;
}

int set_error(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
const char *last_error() { return g_err.c_str(); }

}  // namespace ldso_ba
