// vr_slice.h -- the launch arguments of the slice kernel (vr_slice.hip), shared with the host driver
// (vr_capi.hip do_slice).  Pure data.
#pragma once
#include <stdint.h>

#include "vr_device.h"

namespace vr {

struct SliceParams {
  DevTex tex;             // the source texture (emission / absorption / reflection binding; p null: unbound)
  float origin[3];        // q of pixel (0, 0), sample 0
  float du[3], dv[3];     // q step per output column x / row y
  float dw[3];            // q step per slab sample k
  int32_t width, height;  // W x H
  int32_t samples;        // n >= 1
  int32_t lanes_x;        // a wave's 64 lanes run along x (else along y, the contiguous axis of the output)
  float *out;             // [H, W] column-major
  float *aux;             // likewise, or null
  float *lab;             // likewise, or null
  const uint8_t *labels;  // the resident label bytes, dense, dims ld (null: none)
  int32_t ld[3];
};

}  // namespace vr
