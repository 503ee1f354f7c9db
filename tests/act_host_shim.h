// What the generated eh_jit_act.inc (eh_activation_source) needs from the device side, for the host: tests/test_activations.py compiles
// the generated text with this header in front into one stand-alone program and holds its values against the closures.  The device's own
// eh_tanh / eh_sigmoid / eh_pow (csrc/eh_device.hpp) are stood in for by the C library's.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>

#define __device__
#define __forceinline__ inline
#define __expf(x) std::exp((float)(x))
#define __logf(x) std::log((float)(x))
#define EH_ACT_RECORDED 8

inline float __uint_as_float(unsigned u) { float f; std::memcpy(&f, &u, sizeof f); return f; }
inline float eh_tanh(float x) { return std::tanh(x); }
inline float eh_sigmoid(float x) { return 1.0f / (1.0f + std::exp(-x)); }
inline float eh_pow(float b, float e) { return std::pow(b, e); }
