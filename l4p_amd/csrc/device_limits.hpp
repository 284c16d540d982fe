// What the launchers know about the one target, gfx950, as plain numbers: host-only, no HIP header, so that the pure form selections
// (*_select.hpp) and their CPU tests read the same constants as the launchers (common.hpp includes this file).
#pragma once
#include <stddef.h>

// The LDS of one gfx950 workgroup, static and dynamic together: the most hipFuncSetAttribute grants.  Launchers that choose a kernel
// form by its LDS request, or refuse a geometry, compare against this.
constexpr size_t LDS_DEVICE_LIMIT = 160 * 1024;
