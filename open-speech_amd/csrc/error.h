// The library's exception (an osw.h return code + osw_last_error()'s text) and the argument check.
#pragma once
#include <stdexcept>
#include <string>

#include "../../include/osw.h"

namespace osw {

struct OswError : std::runtime_error {
    int code;
    OswError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define REQUIRE(c, msg) \
    do {                \
        if (!(c)) throw osw::OswError(OSW_EINVAL, msg); \
    } while (0)

}  // namespace osw
