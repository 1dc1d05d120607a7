// capi_error.h — the library's error slot (gfs_last_error), for every unit that reports through it.  Free of HIP (HIPCHK is for
// the units that include the runtime and the ABI's codes themselves).
#pragma once
#include <string>

int gfs_set_error(int code, const std::string &msg);      // host_tables.hip: sets gfs_last_error(), returns code

#define HIPCHK(expr)                                                                                    \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return gfs_set_error(GFS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
    } while (0)
