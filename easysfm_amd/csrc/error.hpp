// Error reporting of libesfm_hip.so, free of HIP so that the host-only units (match_plan.cpp) and their g++ checks share it.
#pragma once

#include "../../include/esfm.h"

namespace esfm {

// Thread-local last-error text behind esfm_last_error().
void set_error(const char *fmt, ...);
const char *get_error();

#define ESFM_REQUIRE(cond, msg)                     \
    do {                                            \
        if (!(cond)) {                              \
            ::esfm::set_error("%s: %s", __func__, msg); \
            return ESFM_ERR_INVALID_ARG;            \
        }                                           \
    } while (0)

}  // namespace esfm
