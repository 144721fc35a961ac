// nice_internal.h -- host entry points shared between translation units of
// libnice_hip.so (not part of the C ABI in include/nice.h).
#pragma once
#include <stdint.h>

#include "../../include/nice.h"

namespace nice {

// nice_decode_batch_dev with the stream lengths optionally already on the host
// (h_stream_len non-null): no device round trip before the first launch.  The
// parse reaches its fixpoint on the device, so with host lengths the call only
// enqueues work.  d_stream_off non-null: a packed batch (include/nice.h) of
// packed_bytes bytes at d_streams, stream f at d_streams + d_stream_off[f]
// (stream_stride unused).
int decode_batch_impl(nice_ctx* ctx, void* stream, const uint8_t* d_streams, uint64_t stream_stride,
                      const uint64_t* d_stream_len, const uint64_t* h_stream_len, uint32_t n_frames,
                      uint32_t w, uint32_t h, uint8_t out_channels, uint8_t* d_px, uint64_t px_stride,
                      uint32_t flags, int32_t* d_status, const uint64_t* d_stream_off = nullptr,
                      uint64_t packed_bytes = 0);

// nice_pack_streams_dev's two launches (nice_packed.hip): the offset scan, which
// also writes *d_status, then the ragged copy on a grid sized from `cus`
// compute units.  Arguments are checked by the caller; never synchronises.
int pack_streams_launch(void* stream, int cus, const uint8_t* d_streams, uint64_t stream_stride,
                        const uint64_t* d_stream_len, uint32_t n_frames, uint8_t* d_packed, uint64_t packed_cap,
                        uint64_t* d_off, int32_t* d_status);

// nice_ctx_reserve; with_packed: also the strided scratch of
// nice_encode_batch_packed_dev (n_frames stream slots).
int ctx_reserve_impl(nice_ctx* ctx, uint32_t n_frames, uint32_t w, uint32_t h, bool with_packed);

}  // namespace nice
