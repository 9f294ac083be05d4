// What the `void*` handles of the C ABI point to, where more than one translation unit needs to know: a reads handle
// (dph_reads_from_*) is taken by the boundary's entry points (host_capi.cpp) and by the test hooks (host_testhooks.cpp).
#pragma once
#include "dph.hpp"

namespace dph {
struct ReadsH {
    ReadSet set;
};
}  // namespace dph
