// nice.hpp -- header-only C++ mirror of the reference codec API over nice.h.
//
//   nice::Image                 image.rs:5-43   (width, height, channels)
//   nice::encode(in, img, channels_out, out)   code.rs:59-64
//   nice::decode(in, channels_out, out) -> Image   code.rs:464-468
//
// Errors: the reference returns io::Error from its writer/reader and panics on
// malformed input; here every failure is a nice::Error carrying the nice.h
// status code.
#ifndef NICE_HPP
#define NICE_HPP
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "nice.h"

namespace nice {

struct Image {
  uint32_t width = 0, height = 0;
  uint8_t channels = 0;
  static Image make(uint32_t w, uint32_t h, uint8_t c) { return Image{w, h, c}; }
};

class Error : public std::runtime_error {
 public:
  Error(int code, const std::string& what)
      : std::runtime_error(what + " failed (status " + std::to_string(code) + ")"), code_(code) {}
  int code() const { return code_; }

 private:
  int code_;
};

inline void check(int rc, const char* what) {
  if (rc != NICE_OK) throw Error(rc, what);
}

// code::encode: appends the stream to `out`.
inline void encode(const std::vector<uint8_t>& in, const Image& img, uint8_t channels_out,
                   std::vector<uint8_t>& out) {
  const size_t base = out.size();
  out.resize(base + nice_encode_bound(img.width, img.height));
  size_t n = 0;
  int rc = nice_encode(in.data(), in.size(), img.width, img.height, img.channels, channels_out,
                       out.data() + base, out.size() - base, &n);
  if (rc != NICE_OK) out.resize(base);
  check(rc, "nice_encode");
  out.resize(base + n);
}

// code::decode: replaces `out` with the pixels (stride = header channels).
// channels_out is accepted and ignored, as in the reference (code.rs never reads it).
inline Image decode(const std::vector<uint8_t>& in, uint8_t /*channels_out*/,
                    std::vector<uint8_t>& out, uint32_t flags = NICE_DEC_ALPHA_FILL_FF) {
  Image img;
  check(nice_peek_header(in.data(), in.size(), &img.width, &img.height, &img.channels),
        "nice_peek_header");
  out.assign((size_t)img.width * img.height * img.channels, 0);
  size_t n = 0;
  check(nice_decode(in.data(), in.size(), out.data(), out.size(), flags, &n), "nice_decode");
  out.resize(n);
  return img;
}

// Owns a device context (scratch arena) for device-resident batches.
class Context {
 public:
  explicit Context(int device = 0) { check(nice_ctx_create(device, &ctx_), "nice_ctx_create"); }
  ~Context() { nice_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  nice_ctx* get() const { return ctx_; }

 private:
  nice_ctx* ctx_ = nullptr;
};

// ---- packed stream batches (nice.h, "packed stream batches") ----
// A packed batch in device memory: the streams back to back at data + off[f]
// (16-byte aligned), off[n] = its size.  The pointers are caller-owned device
// memory; `stream` is a hipStream_t.  All calls are asynchronous.
struct PackedBatch {
  uint8_t* data = nullptr;      // 16-byte aligned, `cap` bytes
  uint64_t cap = 0;
  uint64_t* off = nullptr;      // n + 1
  uint64_t* len = nullptr;      // n
  int32_t* status = nullptr;    // 1: NICE_OK / NICE_E_CAPACITY / NICE_E_ARG, written on the device
  uint32_t n = 0;
};

inline uint64_t packed_bound(uint32_t n_frames, const Image& img) {
  return nice_packed_bound(n_frames, img.width, img.height);
}

// Compacts strided streams (lengths in b.len) into b.
inline void pack_streams(const Context& ctx, void* stream, const uint8_t* d_streams, uint64_t stream_stride,
                         const PackedBatch& b) {
  check(nice_pack_streams_dev(ctx.get(), stream, d_streams, stream_stride, b.len, b.n, b.data, b.cap, b.off,
                              b.status),
        "nice_pack_streams_dev");
}

// Encodes b.n frames of `img` at d_px + f * frame_stride straight into b.
inline void encode_batch_packed(const Context& ctx, void* stream, const uint8_t* d_px, uint64_t frame_stride,
                                const Image& img, uint8_t channels_out, const PackedBatch& b) {
  check(nice_encode_batch_packed_dev(ctx.get(), stream, d_px, frame_stride, b.n, img.width, img.height,
                                     img.channels, channels_out, b.data, b.cap, b.off, b.len, b.status),
        "nice_encode_batch_packed_dev");
}

// Decodes n frames in place from a packed buffer of packed_bytes bytes: frame i
// is the stream at d_off[i] with d_len[i] bytes (any order, repeats allowed).
// h_len: the same lengths on the host, or null.  d_status: n per-frame codes.
inline void decode_packed(const Context& ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                          const uint64_t* d_off, const uint64_t* d_len, const uint64_t* h_len, uint32_t n,
                          const Image& img, uint8_t out_channels, uint8_t* d_px, uint64_t px_stride,
                          int32_t* d_status, uint32_t flags = NICE_DEC_ALPHA_FILL_FF) {
  check(nice_decode_packed_dev(ctx.get(), stream, d_packed, packed_bytes, d_off, d_len, h_len, n, img.width,
                               img.height, out_channels, d_px, px_stride, flags, d_status),
        "nice_decode_packed_dev");
}

// ---- image sets: tensor output (nice.h, "image sets: tensor output") ----
enum class TensorType : uint32_t { F32 = NICE_TENSOR_F32, F16 = NICE_TENSOR_F16, BF16 = NICE_TENSOR_BF16 };
enum class TensorLayout : uint32_t { Planar = NICE_TENSOR_PLANAR, Interleaved = NICE_TENSOR_INTERLEAVED };

// An encoded set: the packed tiles in device memory, every table on the host.
struct SetTables {
  const uint8_t* d_packed = nullptr;   // 16-byte aligned
  uint64_t packed_bytes = 0;
  const uint64_t* off = nullptr;       // n + 1
  const uint64_t* len = nullptr;       // n
  const uint8_t* kind = nullptr;       // n
  const uint32_t* w = nullptr;         // K
  const uint32_t* h = nullptr;         // K
  uint32_t K = 0, tile_w = 0, tile_h = 0;
};

// M windows {image, x0, y0, rw, rh} and where each goes: base pointers (device
// memory), pitches in elements, flip (null: none) as nice.h defines them.
struct TensorWindows {
  const uint32_t* win = nullptr;       // 5 * M
  const uint8_t* flip = nullptr;       // M, or null
  void* const* out = nullptr;          // M
  const uint64_t* row_pitch = nullptr;     // M
  const uint64_t* plane_pitch = nullptr;   // M (planar only)
  uint32_t M = 0;
};

// element = fmaf(byte, scale[c], bias[c]), stored as `type`
struct TensorAffine {
  float scale[3] = {1.0f / 255.0f, 1.0f / 255.0f, 1.0f / 255.0f};
  float bias[3] = {0.0f, 0.0f, 0.0f};
};

// Decodes the windows of a set straight into normalised tensors (colour only).
// d_status: one code per slot (nice_set_select), written on the device.
inline void decode_set_tensor(const Context& ctx, void* stream, const SetTables& s, const TensorWindows& t,
                              TensorType type, TensorLayout layout, const TensorAffine& a, int32_t* d_status,
                              uint32_t flags = NICE_DEC_ALPHA_FILL_FF) {
  check(nice_decode_set_tensor_dev(ctx.get(), stream, s.d_packed, s.packed_bytes, s.off, s.len, s.kind, s.w, s.h, s.K,
                                   s.tile_w, s.tile_h, t.win, t.flip, t.out, t.row_pitch, t.plane_pitch, t.M,
                                   (uint32_t)type, (uint32_t)layout, a.scale, a.bias, flags, d_status),
        "nice_decode_set_tensor_dev");
}

// ---- image sets: resized tensor output (nice.h, "image sets: resized tensor output") ----
// decode_set_tensor with every window resampled to out_h x out_w (fixed-point
// bilinear, no antialiasing): t.out[j] holds out_h x out_w elements per channel.
// antialias: a reducing axis takes the integer triangle filter of nice.h,
// "image sets: antialiased resized tensor output" (nice_decode_set_resized_aa_dev).
inline void decode_set_resized(const Context& ctx, void* stream, const SetTables& s, const TensorWindows& t,
                               uint32_t out_w, uint32_t out_h, TensorType type, TensorLayout layout,
                               const TensorAffine& a, int32_t* d_status, uint32_t flags = NICE_DEC_ALPHA_FILL_FF,
                               bool antialias = false) {
  if (antialias) {
    check(nice_decode_set_resized_aa_dev(ctx.get(), stream, s.d_packed, s.packed_bytes, s.off, s.len, s.kind, s.w, s.h,
                                         s.K, s.tile_w, s.tile_h, t.win, t.flip, out_w, out_h, t.out, t.row_pitch,
                                         t.plane_pitch, t.M, (uint32_t)type, (uint32_t)layout, a.scale, a.bias, flags,
                                         d_status),
          "nice_decode_set_resized_aa_dev");
    return;
  }
  check(nice_decode_set_resized_dev(ctx.get(), stream, s.d_packed, s.packed_bytes, s.off, s.len, s.kind, s.w, s.h, s.K,
                                    s.tile_w, s.tile_h, t.win, t.flip, out_w, out_h, t.out, t.row_pitch,
                                    t.plane_pitch, t.M, (uint32_t)type, (uint32_t)layout, a.scale, a.bias, flags,
                                    d_status),
        "nice_decode_set_resized_dev");
}

}  // namespace nice
#endif  // NICE_HPP
