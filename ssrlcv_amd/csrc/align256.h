// ssrlcv_amd/csrc/align256.h -- the parts of a workspace start on 256-byte boundaries: the one round-up to it.
#pragma once
#include <stddef.h>

inline size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }
