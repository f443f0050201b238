// The library's error hook: the message vge_last_error() returns (thread-local, defined in vge_api.cpp).
#pragma once
#include <string>

namespace vge {
void set_last_error(const std::string& msg);
}  // namespace vge
