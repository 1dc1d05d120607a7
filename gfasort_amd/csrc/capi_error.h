// capi_error.h — the library's error slot (gfs_last_error), for every unit that reports through it.  Free of HIP.
#pragma once
#include <string>

int gfs_set_error(int code, const std::string &msg);      // host_tables.hip: sets gfs_last_error(), returns code
