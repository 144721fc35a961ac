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

// The first of the two alone: d_off (n_frames + 1) and *d_status from the lengths.
int pack_offsets_launch(void* stream, uint64_t stream_stride, const uint64_t* d_stream_len, uint32_t n_frames,
                        uint64_t packed_cap, uint64_t* d_off, int32_t* d_status);

// ---- tiled images (nice_tiles.hip) -----------------------------------------
// Arguments are checked by the callers (nice_capi.hip); every launch is
// asynchronous on `stream`.  NICE_E_ARG: the grid would not fit a launch.
// Image -> nx * ny dense tiles with clamped-coordinate padding.
int tiles_split_launch(void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t channels,
                       uint32_t tile_w, uint32_t tile_h, uint32_t nx, uint32_t ny, uint8_t* d_tiles,
                       uint64_t tile_stride);
// Slot i (at d_tiles + i * tile_stride, or d_tiles + d_src_off[i]) holds tile
// d_tile_idx[i]; its part inside the rectangle and the image goes to the
// window.  A slot with d_slot_status[i] != 0 (d_slot_status may be null) is
// skipped.  fill: byte +3 of a 4-byte output pixel when the slots hold 3.
int tiles_merge_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint64_t* d_src_off,
                       const uint32_t* d_tile_idx, const int32_t* d_slot_status, uint32_t n_slots, uint32_t w,
                       uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t nx, uint32_t ny, uint32_t x0, uint32_t y0,
                       uint32_t rw, uint32_t rh, uint32_t tile_channels, uint32_t out_channels, uint32_t fill,
                       uint8_t* d_out, uint64_t out_pitch);
// d_kind[t] = 0 if bytes +0..+2 of every pixel agree and d_status[t] == 0, else 1.
int tiles_compare_launch(void* stream, const uint8_t* d_a, uint64_t stride_a, const uint8_t* d_b, uint64_t stride_b,
                         uint32_t channels, uint32_t n, uint32_t npx, const int32_t* d_status, uint8_t* d_kind);
// Tiles with d_kind[t] == 1: slot t = the tile's RGB, d_len[t] = 3 * npx.
int tiles_store_raw_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, uint32_t channels, uint32_t n,
                           uint32_t npx, const uint8_t* d_kind, uint8_t* d_slots, uint64_t slot_stride,
                           uint64_t* d_len);
// d_out[d_pos[i]] = d_st[i]
int tiles_scatter_status_launch(void* stream, const int32_t* d_st, const uint32_t* d_pos, uint32_t n, int32_t* d_out);

// ---- the alpha batch of a tiled image (nice_tiles.hip) -----------------------
// aw3 = 3 * ceil(tile_w / 3): bytes per row of a tile's triplet image.
// d_lo[t], d_hi[t] = min, max of byte +3 over tile t of an RGBA image (both preset by the call).
int alpha_range_launch(void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t tile_w,
                       uint32_t tile_h, uint32_t nx, uint32_t ny, uint32_t* d_lo, uint32_t* d_hi);
// The triplet image of tile d_list[i] dense at d_trip + i * trip_stride, i < m.
int alpha_gather_launch(void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t tile_w,
                        uint32_t tile_h, uint32_t nx, const uint32_t* d_list, uint32_t m, uint8_t* d_trip,
                        uint64_t trip_stride);
// Stream i is stored raw where d_vk[i] != 0 (the verify compare) or
// d_mlen[i] >= tile_w * tile_h: d_vk[i] becomes that verdict, slot i the plane,
// d_mlen[i] the stored length; d_akind / d_alen of tile d_list[i] are written,
// and the slot's bytes from the length to the next multiple of 16 zeroed.
int alpha_store_launch(void* stream, const uint8_t* d_trip, uint64_t trip_stride, uint32_t tile_w, uint32_t tile_h,
                       const uint32_t* d_list, uint32_t m, uint8_t* d_vk, uint64_t* d_mlen, uint8_t* d_slots,
                       uint64_t slot_stride, uint8_t* d_akind, uint64_t* d_alen);
// Slot i (16-byte aligned, zero pad bytes) to d_packed + d_off[d_list[i]]; nothing at or past packed_cap.
int alpha_pack_launch(void* stream, const uint8_t* d_slots, uint64_t slot_stride, const uint64_t* d_mlen,
                      const uint32_t* d_list, uint32_t m, const uint64_t* d_off, uint8_t* d_packed, uint64_t packed_cap);
// Byte +3 of the window's RGBA pixels.  Slot i holds tile d_tile_idx[i] of
// d_kind[i]: 0 the decoded triplet image d_src[i] (skipped where its
// d_dec_status is nonzero), 1 the plane at d_packed + d_src[i], 2 the constant d_src[i].
int alpha_merge_launch(void* stream, const uint8_t* d_dec, uint64_t dec_stride, const int32_t* d_dec_status,
                       const uint8_t* d_packed, const uint64_t* d_src, const uint8_t* d_kind, const uint32_t* d_tile_idx,
                       uint32_t n_slots, uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t nx,
                       uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh, uint8_t* d_out, uint64_t out_pitch);

// ---- image sets (nice_sets.hip) ----------------------------------------------
// Device descriptor tables, built and uploaded by the callers (nice_capi.hip).
// mode: the best move mode (0 bytes, 1 dwords, 2 16 bytes) the member's own
// base, pitch and, for a window, x0 allow; the kernels take the lower of it
// and what the tile array allows.
struct SetImage {
  const uint8_t* img;
  uint64_t pitch;
  uint32_t w, h, nx;
  uint32_t first;   // the image's first global tile; first of entry 0 is 0, ascending
  uint32_t mode, pad;
};
struct SetWindow {
  uint8_t* out;
  uint64_t pitch;
  uint32_t x0, y0, rw, rh;      // the rectangle, inside its image
  uint32_t w, h, nx, n_tiles;   // of that image
  uint32_t mode, pad;
};
uint32_t set_image_mode(const uint8_t* d_img, uint64_t row_pitch);
uint32_t set_window_mode(const uint8_t* d_out, uint64_t out_pitch, uint32_t x0);
// K images -> n dense tiles (global tile order) with clamped-coordinate padding.
int set_split_launch(void* stream, const SetImage* d_imgs, uint32_t K, uint32_t n, uint32_t channels, uint32_t tile_w,
                     uint32_t tile_h, uint8_t* d_tiles, uint64_t tile_stride);
// Slot i (at d_tiles + i * tile_stride, or d_tiles + d_src_off[i]) holds tile
// d_slot_tile[i] of the image of window d_slot_win[i]; its part inside that
// window goes there.  Skipped: a slot with d_slot_status[i] != 0 (may be null),
// a window index >= n_wins, a tile index outside the image.
int set_merge_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint64_t* d_src_off,
                     const uint32_t* d_slot_win, const uint32_t* d_slot_tile, const int32_t* d_slot_status,
                     uint32_t n_slots, const SetWindow* d_wins, uint32_t n_wins, uint32_t tile_w, uint32_t tile_h,
                     uint32_t tile_channels, uint32_t out_channels, uint32_t fill);

// ---- image sets: tensor output (nice_sets_tensor.hip) --------------------------
// A window of the tensor merge: element (c, y, x) at out + c * plane_pitch +
// y * row_pitch + x (planar) or out + y * row_pitch + 3 * x + c (interleaved),
// pitches in elements.  mode: log2 of the pixels a lane converts and stores as
// one vector per plane (0: element by element), the best the window's base,
// pitches, element size and x0 (flipped: x0 + rw) allow.
struct SetTensorWindow {
  void* out;
  uint64_t row_pitch, plane_pitch;
  uint32_t x0, y0, rw, rh;      // the rectangle, inside its image
  uint32_t w, h, nx, n_tiles;   // of that image
  uint32_t mode, flip;
};
uint32_t set_tensor_elem_bytes(uint32_t dtype);   // 0: unknown dtype
uint32_t set_tensor_window_mode(const void* d_out, uint64_t row_pitch, uint64_t plane_pitch, uint32_t x0, uint32_t rw,
                                bool flip, uint32_t dtype);   // plane_pitch 0: interleaved
// set_merge_launch's slots and skips; every window element takes
// fmaf(byte, scale[c], bias[c]) of its pixel's bytes +0..+2, converted to dtype.
int set_merge_tensor_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint64_t* d_src_off,
                            const uint32_t* d_slot_win, const uint32_t* d_slot_tile, const int32_t* d_slot_status,
                            uint32_t n_slots, const SetTensorWindow* d_wins, uint32_t n_wins, uint32_t tile_w,
                            uint32_t tile_h, uint32_t tile_channels, uint32_t dtype, uint32_t layout, const float* scale,
                            const float* bias);

// ---- image sets: resized tensor output (nice_sets_resize.hip) -------------------
// A window of the resize merge: its out_h x out_w elements per channel laid out
// as SetTensorWindow's; its slots are slot_first + (ty - ty0) * ntx + (tx - tx0)
// for the tiles tx0 <= tx < tx0 + ntx, ty0 <= ty of its image.  mode: log2 of
// the consecutive output columns a lane stores as one vector per plane, the
// best the base, the pitches and the element size allow.
struct SetResizeWindow {
  void* out;
  uint64_t row_pitch, plane_pitch;
  uint32_t x0, y0, rw, rh;      // the rectangle, inside its image
  uint32_t tx0, ty0, ntx;       // its tiles
  uint32_t slot_first;
  uint32_t mode, flip;
};
uint32_t set_resize_window_mode(const void* d_out, uint64_t row_pitch, uint64_t plane_pitch, uint32_t dtype);
// Every element of the n_wins windows from the slots its taps fall in (d_src[p]
// as slot_position_sources gives it: dense slots at d_tiles + value *
// tile_stride, dwords; raw slots at d_packed + value).  An element with a tap
// in a slot whose d_slot_status[p] != 0 (may be null) or whose source is
// neither dense nor raw is not written.  One launch.
int set_resize_tensor_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint8_t* d_packed,
                             const uint64_t* d_src, const int32_t* d_slot_status, const SetResizeWindow* d_wins,
                             uint32_t n_wins, uint32_t tile_w, uint32_t tile_h, uint32_t out_w, uint32_t out_h,
                             uint32_t dtype, uint32_t layout, const float* scale, const float* bias);

// ---- image sets: antialiased resized tensor output (nice_sets_resize_aa.hip) ----
// A window of the antialiased resize: SetResizeWindow's output and slots, and
// where the weight tables of its axes begin, in entries of 16 bits (a reducing
// axis of n_in pixels has 2 n_in entries, any other none).
struct SetResizeAaWindow {
  void* out;
  uint64_t row_pitch, plane_pitch;
  uint32_t x0, y0, rw, rh;      // the rectangle, inside its image
  uint32_t tx0, ty0, ntx;       // its tiles
  uint32_t slot_first;
  uint32_t wcol, wrow;          // the tables of its columns and of its rows
  uint32_t flip, pad;
};
uint64_t set_resize_aa_table_entries(uint32_t n_in, uint32_t n_out);
// set_resize_tensor_launch's slots and skips, by the triangle filter of
// nice_resize.hpp.  d_weights: room for the tables of all windows;
// max_reducing: the longest reducing axis among them (0: none reduces).  Two
// launches: the weight tables, then the filter.
int set_resize_aa_tensor_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint8_t* d_packed,
                                const uint64_t* d_src, const int32_t* d_slot_status, const SetResizeAaWindow* d_wins,
                                uint32_t n_wins, uint16_t* d_weights, uint32_t max_reducing, uint32_t tile_w,
                                uint32_t tile_h, uint32_t out_w, uint32_t out_h, uint32_t dtype, uint32_t layout,
                                const float* scale, const float* bias);

// ---- the alpha batch of an image set (nice_sets.hip) --------------------------
// The set forms of alpha_range_launch, alpha_gather_launch and alpha_merge_launch
// above: tiles are global tile indices, their images (RGBA) come from d_imgs.
// d_lo[g], d_hi[g] = min, max of byte +3 over global tile g, g < n (both preset by the call).
int set_alpha_range_launch(void* stream, const SetImage* d_imgs, uint32_t K, uint32_t n, uint32_t tile_w,
                           uint32_t tile_h, uint32_t* d_lo, uint32_t* d_hi);
// The triplet image of global tile d_list[i] dense at d_trip + i * trip_stride, i < m.
int set_alpha_gather_launch(void* stream, const SetImage* d_imgs, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                            const uint32_t* d_list, uint32_t m, uint8_t* d_trip, uint64_t trip_stride);
// Byte +3 of the windows' RGBA pixels.  Slot i holds tile d_slot_tile[i] of the
// image of window d_slot_win[i], of d_kind[i] with source d_src[i] as for
// alpha_merge_launch.  Skipped: a coded slot whose d_dec_status is nonzero, a
// window index >= n_wins, a tile index outside the image.
int set_alpha_merge_launch(void* stream, const uint8_t* d_dec, uint64_t dec_stride, const int32_t* d_dec_status,
                           const uint8_t* d_packed, const uint64_t* d_src, const uint8_t* d_kind,
                           const uint32_t* d_slot_win, const uint32_t* d_slot_tile, uint32_t n_slots,
                           const SetWindow* d_wins, uint32_t n_wins, uint32_t tile_w, uint32_t tile_h);

// nice_ctx_reserve; with_packed: also the strided scratch of
// nice_encode_batch_packed_dev (n_frames stream slots).
int ctx_reserve_impl(nice_ctx* ctx, uint32_t n_frames, uint32_t w, uint32_t h, bool with_packed);

}  // namespace nice
