// nice_dec_rec.hpp -- the decoder's per-pixel record: what the record writers
// (dec_emit, dec_place: nice_decode.hip) store and the row kernels
// (nice_rows.hip) read -- its layout and arithmetic are nice_dec_event.hpp's,
// which a host compiler reads too -- and the frame status both sides set.
// Device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nice_dec_event.hpp"
#include "nice_format.h"

namespace nice {

// first error of a frame wins
__device__ __forceinline__ void set_status(int32_t* st, int32_t code) {
  atomicCAS(reinterpret_cast<int*>(st), 0, code);
}

}  // namespace nice
