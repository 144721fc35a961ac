/* nice.h -- C ABI of the MI355X-native NICE2 codec (libnice_hip.so).
 *
 * Drop-in boundary for the reference's codec entry points:
 *   code::encode  /root/reference/src/code.rs:59-64
 *       pub fn encode<W: io::Write>(input_bytes: &[u8], image_header: Image,
 *                                   channels_out: u8, output_writer: &mut W)
 *   code::decode  /root/reference/src/code.rs:464-468
 *       pub fn decode<R: io::Read>(image_reader: &mut R, channels_out: u8,
 *                                  output_vec: &mut Vec<u8>) -> io::Result<Image>
 *   image::Image::new  /root/reference/src/image.rs:22-43 (width, height, channels)
 *
 * Plain pointers and sizes only.  Every function returns a status code (0 = ok,
 * negative = error) and never aborts, where the reference panics/aborts
 * (Cargo.toml:16 panic = "abort").  Buffers are caller-owned.  Functions taking a
 * nice_ctx are thread-safe per context; the context-free functions use an
 * internal per-device context guarded by a mutex.
 *
 * Frame size cap: every encode/decode entry point (and the band API) refuses a
 * frame of more than 2^30 pixels (w * h > 1073741824, e.g. 32768 x 32768) with
 * NICE_E_ARG.  code::encode has no such limit (code.rs:59-64, 87); the cap keeps
 * pixel indices and Huffman counts 32-bit on the device: a stream's symbol
 * total is at most 3 per pixel (SC_RGB), i.e. < 3 * 2^30 < 2^32, which the
 * heap's 32-bit count keys and merge sums hold exactly (tests/test_tables.py
 * covers totals up to 3 * 2^30).  A 2^30-pixel RGBA frame is 4 GiB of input.
 */
#ifndef NICE_H
#define NICE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  NICE_OK = 0,
  NICE_E_ARG = -1,          /* bad argument (sizes, channels, alignment) */
  NICE_E_HIP = -2,          /* HIP runtime failure */
  NICE_E_NODEV = -3,        /* no usable gfx950 device */
  NICE_E_CAPACITY = -4,     /* output buffer too small */
  NICE_E_FORMAT = -5,       /* malformed stream: the reference would panic here */
  NICE_E_UNSUPPORTED = -6   /* stream outside the reference decoder's domain (see flags) */
};

/* nice_decode flags */
#define NICE_DEC_STRICT_REFERENCE 0x1u /* fail wherever the reference decoder would fail */
#define NICE_DEC_ALPHA_FILL_FF 0x2u    /* 4-channel output: write A = 255 */
/* Tolerant table header: repairs the length field a
 * spilled 5-bit max (> 31) corrupts in the reference writer, and decodes with
 * the <= 31-bit codes.  Streams of small or very flat images (every max > 31
 * because zero-count symbols chain deep in the Huffman merge) decode only
 * with this flag; the reference decoder cannot decode them.  Ignored with
 * NICE_DEC_STRICT_REFERENCE. */
#define NICE_DEC_TOLERANT_HEADER 0x4u

typedef struct nice_ctx nice_ctx;

/* Library / device queries. */
const char* nice_version(void);
int nice_device_count(void);

/* Upper bound of an encoded stream for a w x h image (any channels). */
size_t nice_encode_bound(uint32_t w, uint32_t h);

/* Replaces code::encode (code.rs:59-64): host pixels in, host stream out.
 * px: w*h pixels of `channels` (3 or 4) bytes; only bytes +0..+2 of each pixel
 * are coded (code.rs:197,215-217).  channels_out is written to header byte 12
 * (code.rs:84).  *out_len receives the stream length. */
int nice_encode(const uint8_t* px, size_t px_len, uint32_t w, uint32_t h, uint8_t channels,
                uint8_t channels_out, uint8_t* out, size_t out_cap, size_t* out_len);

/* Parses the 13-byte file header (code.rs:469-483). */
int nice_peek_header(const uint8_t* s, size_t len, uint32_t* w, uint32_t* h, uint8_t* ch);

/* Replaces code::decode (code.rs:464-468): host stream in, host pixels out.
 * Output pixel stride = header channels byte (3: RGB; 4: RGB + alpha byte, 255
 * with NICE_DEC_ALPHA_FILL_FF, else 0).  *px_len receives w*h*channels. */
int nice_decode(const uint8_t* s, size_t len, uint8_t* px_out, size_t cap, uint32_t flags,
                size_t* px_len);

/* ---- context API: device buffers, HIP streams (passed as void*), batches ---- */
int nice_ctx_create(int device, nice_ctx** out);
void nice_ctx_destroy(nice_ctx* ctx);
/* Pre-size scratch so later batch calls allocate nothing (graph-capturable);
 * this includes nice_encode_batch_packed_dev's n_frames stream slots. */
int nice_ctx_reserve(nice_ctx* ctx, uint32_t n_frames, uint32_t w, uint32_t h);

/* Encode n_frames same-shape frames resident in device memory.
 * d_px: frame f at d_px + f*frame_stride (4-byte aligned for channels == 4).
 * d_out: frame f's stream at d_out + f*out_stride (4-byte aligned, out_stride a
 * multiple of 4 and >= nice_encode_bound(w, h)); d_out_len[f] = its length.
 * Asynchronous on `stream`. */
int nice_encode_batch_dev(nice_ctx* ctx, void* stream, const uint8_t* d_px, uint64_t frame_stride,
                          uint32_t n_frames, uint32_t w, uint32_t h, uint8_t channels,
                          uint8_t channels_out, uint8_t* d_out, uint64_t out_stride,
                          uint64_t* d_out_len);

/* Decode n_frames streams resident in device memory (all w x h).
 * d_streams: stream f at d_streams + f*stream_stride, d_stream_len[f] bytes.
 * d_px: frame f written at d_px + f*px_stride with out_channels (3 or 4) bytes
 * per pixel.  d_status[f] = NICE_OK or a negative code.  Asynchronous: the
 * parse fixpoint is reached on the device; the call reads the lengths back
 * first (they size the scratch), i.e. waits for the work queued on `stream`
 * before it, never for the decode itself. */
int nice_decode_batch_dev(nice_ctx* ctx, void* stream, const uint8_t* d_streams,
                          uint64_t stream_stride, const uint64_t* d_stream_len, uint32_t n_frames,
                          uint32_t w, uint32_t h, uint8_t out_channels, uint8_t* d_px,
                          uint64_t px_stride, uint32_t flags, int32_t* d_status);
/* The same with the lengths also on the host (h_stream_len[f] == d_stream_len[f]):
 * the call only enqueues work, it never waits for the device. */
int nice_decode_batch_dev_hl(nice_ctx* ctx, void* stream, const uint8_t* d_streams,
                             uint64_t stream_stride, const uint64_t* d_stream_len,
                             const uint64_t* h_stream_len, uint32_t n_frames, uint32_t w, uint32_t h,
                             uint8_t out_channels, uint8_t* d_px, uint64_t px_stride, uint32_t flags,
                             int32_t* d_status);

/* ---- packed stream batches ----
 * A strided batch spends nice_encode_bound(w, h) bytes per frame, the size of
 * the raw frame.  The packed form keeps the same streams, bit for bit, back to
 * back in one device buffer with an offset table.  Layout, for n streams of
 * len[f] bytes (align16(x) = x rounded up to a multiple of 16):
 *   off[0] = 0
 *   off[f + 1] = off[f] + align16(len[f])
 *   off[n] = the packed size
 *   stream f occupies packed[off[f] .. off[f] + len[f])
 *   the pad bytes up to off[f + 1] are zero (a packed buffer is a pure function
 *   of its streams); a zero-length stream occupies nothing
 * d_packed is 16-byte aligned, so every stream is.  The offset table is n + 1
 * u64 in device memory.
 *
 * What the decoder reads: of a stream at offset o with length len, only bytes
 * [o, o + len) -- its 16-byte refills are issued only for quads that end at or
 * before len rounded down to 4, and the last partial quad is read byte by byte
 * below len (positions past len repeat the last byte, as in the strided form).
 * No pad byte and no byte of a neighbouring stream is ever loaded, so no tail
 * padding is needed: packed_bytes = off[n] exactly, and nice_packed_bound()
 * has no slack beyond the per-stream alignment.
 *
 * All three calls are asynchronous on `stream`. */
/* Worst-case packed size of n_frames w x h streams. */
uint64_t nice_packed_bound(uint32_t n_frames, uint32_t w, uint32_t h);
/* Compacts a strided batch (stream f at d_streams + f*stream_stride, both
 * multiples of 4; d_stream_len[f] <= stream_stride bytes) into d_packed
 * (16-byte aligned, packed_cap bytes).  Never synchronises: the lengths are
 * only read on the device.  d_off (n_frames + 1) is always written in full, so
 * d_off[n_frames] is the size the call needed.  *d_status:
 *   NICE_OK          every stream copied, pads zeroed
 *   NICE_E_CAPACITY  d_off[n_frames] > packed_cap: no byte at or past packed_cap
 *                    is written; streams that end at or before packed_cap
 *                    rounded down to 16 are complete
 *   NICE_E_ARG       some d_stream_len[f] > stream_stride: that stream counts
 *                    as empty in d_off and is not copied
 * Source bytes at or beyond d_stream_len[f] rounded up to 4 are not read. */
int nice_pack_streams_dev(nice_ctx* ctx, void* stream, const uint8_t* d_streams, uint64_t stream_stride,
                          const uint64_t* d_stream_len, uint32_t n_frames, uint8_t* d_packed,
                          uint64_t packed_cap, uint64_t* d_off /* n_frames + 1 */, int32_t* d_status /* 1 */);
/* nice_encode_batch_dev into a strided scratch owned and reused by the context
 * (n_frames slots of nice_encode_bound(w, h); nice_ctx_reserve pre-sizes it),
 * then nice_pack_streams_dev into d_packed.  d_out_len[f] = stream f's length;
 * d_off, *d_status as above. */
int nice_encode_batch_packed_dev(nice_ctx* ctx, void* stream, const uint8_t* d_px, uint64_t frame_stride,
                                 uint32_t n_frames, uint32_t w, uint32_t h, uint8_t channels,
                                 uint8_t channels_out, uint8_t* d_packed, uint64_t packed_cap, uint64_t* d_off,
                                 uint64_t* d_out_len, int32_t* d_status);
/* nice_decode_batch_dev reading stream f in place at d_packed + d_off[f]
 * (d_packed 16-byte aligned).  d_off has n_frames entries in any order, repeats
 * allowed: gather d_off / d_stream_len to decode a subset of a batch.  A frame
 * whose d_off[f] is not a multiple of 16, or with d_off[f] + d_stream_len[f] >
 * packed_bytes, gets NICE_E_ARG in d_status[f] before any byte of it is read;
 * the other frames decode.  h_stream_len: the lengths on the host (the call
 * then only enqueues work), or NULL (they are read back first, as by
 * nice_decode_batch_dev). */
int nice_decode_packed_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                           const uint64_t* d_off, const uint64_t* d_stream_len, const uint64_t* h_stream_len,
                           uint32_t n_frames, uint32_t w, uint32_t h, uint8_t out_channels, uint8_t* d_px,
                           uint64_t px_stride, uint32_t flags, int32_t* d_status);

/* ---- tiled images ----
 * One image cut into independent tiles, coded as one packed batch: a single
 * large image decodes on the whole device instead of row by row on one compute
 * unit, a rectangle decodes from the tiles it touches alone, and the result is
 * lossless for every input (below).
 *
 * Geometry.  The image is w x h (w, h >= 1, w * h <= 2^30) with `channels` 3
 * or 4; the tile is tile_w x tile_h, 2 <= tile_w, tile_h <= 8192.
 *   nx = ceil(w / tile_w), ny = ceil(h / tile_h), n = nx * ny
 *   tile t = ty * nx + tx covers image pixels [tx*tile_w, ..) x [ty*tile_h, ..)
 * Every tile is coded at the full tile_w x tile_h, edge tiles and images
 * smaller than one tile included: a position outside the image takes the
 * pixel at the clamped coordinate (min(x, w - 1), min(y, h - 1)).  n times the
 * 1024-pixel encoder tiles of one tile must stay below 2^32 (the batch
 * encoder's work counter).  Anything else is NICE_E_ARG.
 * As everywhere in this codec only bytes +0..+2 of a pixel are coded: the
 * colour batch does not preserve alpha either.  Byte +3 of an RGBA image is
 * kept by a second packed batch beside it ("alpha", below).
 *
 * Layout.  The n tiles are a packed batch (above): d_packed, off[n + 1],
 * len[n], plus kind[n] (u8).  kind 0: an ordinary NICE stream, byte for byte
 * what nice_encode gives for the padded tile's pixels.  kind 1: the tile's raw
 * RGB, tile_w * tile_h * 3 bytes in row-major order.  Raw tiles exist because
 * the format cannot carry every table its encoder builds: a Huffman table
 * whose longest code exceeds 128 bits gets a header no decoder can read, and
 * small, smooth tiles do produce such tables.  The encoder therefore decodes
 * every tile back, compares, and stores the failing ones raw. */
/* Validates the geometry; *nx, *ny receive the grid. */
int nice_tile_grid(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t* nx, uint32_t* ny);
/* nice_packed_bound(nx * ny, tile_w, tile_h): always enough for d_packed (a
 * raw tile is smaller than nice_encode_bound).  0 for a bad geometry. */
uint64_t nice_tiled_bound(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h);
/* The half-open tile range [tx0, tx1) x [ty0, ty1) that the rectangle
 * [x0, x0 + rw) x [y0, y0 + rh) touches.  An empty rectangle or one that
 * leaves the image is NICE_E_ARG. */
int nice_tile_select(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t rw,
                     uint32_t rh, uint32_t* tx0, uint32_t* ty0, uint32_t* tx1, uint32_t* ty1);
/* Image -> tiles.  d_img: rows of w pixels, row y at d_img + y*row_pitch
 * (row_pitch >= w*channels; any alignment).  Tile t is written dense at
 * d_tiles + t*tile_stride (tile_stride >= tile_w*tile_h*channels), padded by
 * the clamp rule.  RGBA with tile_w % 4 == 0 and 16-byte aligned d_img,
 * row_pitch, d_tiles and tile_stride moves 16 bytes per lane; other RGBA with
 * 4-byte alignment one dword per pixel; everything else bytes.  Asynchronous. */
int nice_tiles_split_dev(nice_ctx* ctx, void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h,
                         uint8_t channels, uint32_t tile_w, uint32_t tile_h, uint8_t* d_tiles, uint64_t tile_stride);
/* Tiles -> window.  Slot i (d_tiles + i*tile_stride, tile_channels bytes per
 * pixel) holds tile d_tile_idx[i]; d_tile_idx is device memory, slots in any
 * order, an index >= nx*ny is skipped.  For each slot the intersection of its
 * tile, the rectangle (inside the image, as for nice_tile_select) and the
 * image is written to d_out + (y - y0)*out_pitch + (x - x0)*out_channels
 * (out_pitch >= rw*out_channels).  Nothing outside the rw x rh window is
 * written, and no padding.  tile_channels 3 -> out_channels 4 writes `alpha`
 * as byte +3; 4 -> 3 drops it.  The 16-byte path needs RGBA on both sides,
 * tile_w % 4 == 0, x0 % 4 == 0 and 16-byte aligned bases, stride and pitch.
 * Asynchronous. */
int nice_tiles_merge_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                         const uint32_t* d_tile_idx, uint32_t n_slots, uint8_t tile_channels, uint32_t w, uint32_t h,
                         uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh,
                         uint8_t out_channels, uint8_t alpha, uint8_t* d_out, uint64_t out_pitch);
/* Encodes one device-resident image as n tiles: split into context scratch,
 * nice_encode_batch_dev into the context's strided stream slots, decode of
 * every tile with NICE_DEC_TOLERANT_HEADER, compare with the split tiles
 * (bytes +0..+2), raw RGB over the slot of every tile that failed or differed,
 * then the pack into d_packed (16-byte aligned, packed_cap bytes;
 * nice_tiled_bound() always suffices).  d_off (n + 1 u64) and *d_status are
 * written as by nice_encode_batch_packed_dev, d_len[t] (n u64) = tile t's
 * length, d_kind[t] (n u8) = 0 coded, 1 raw; all device memory.
 * The call waits once for the work it queued itself (the stream lengths size
 * the verify decode's scratch, as in nice_decode_batch_dev); the verify
 * decode, compare, raw store and pack are only enqueued.
 * Scratch, owned and reused by the context, nice_ctx_reserve does not
 * pre-size it: the split tiles and the decoded tiles (padded image x channels
 * each), the stream slots (nice_encode_bound per tile, about 4 bytes per
 * pixel) and the batch encoder's and decoder's own scratch. */
int nice_encode_tiled_dev(nice_ctx* ctx, void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h,
                          uint8_t channels, uint8_t channels_out, uint32_t tile_w, uint32_t tile_h, uint8_t* d_packed,
                          uint64_t packed_cap, uint64_t* d_off /* n + 1 */, uint64_t* d_len /* n */,
                          uint8_t* d_kind /* n */, int32_t* d_status /* 1 */);
/* Decodes the rectangle [x0, x0 + rw) x [y0, y0 + rh) of a tiled image into
 * d_out (row pitch out_pitch >= rw*out_channels, out_channels 3 or 4).
 * h_off, h_len, h_kind: the tables of all n tiles in host memory (h_off needs
 * n entries).  Only the tiles the rectangle touches are read: coded tiles are
 * decoded in place from d_packed (16-byte aligned) into context scratch, raw
 * tiles are expanded from their 3-byte pixels, and both are merged into the
 * window.  The tolerant table header is always on; NICE_DEC_ALPHA_FILL_FF is
 * honoured (raw tiles included); NICE_DEC_STRICT_REFERENCE is NICE_E_ARG.
 * d_status: one entry per selected tile, row-major over [ty0, ty1) x [tx0, tx1)
 * of nice_tile_select.  A tile whose status is not NICE_OK leaves its pixels
 * of the window untouched; the others are written.  Per tile: an offset that
 * is not a multiple of 16 or off + len > packed_bytes is NICE_E_ARG, a kind
 * other than 0 or 1 or a raw length other than tile_w*tile_h*3 NICE_E_FORMAT,
 * a coded tile reports its decode status.
 * The call uploads the gathered tables of the selected tiles (a few KB) and
 * otherwise only enqueues work. */
int nice_decode_tiled_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                          const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind, uint32_t w, uint32_t h,
                          uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh,
                          uint8_t out_channels, uint8_t* d_out, uint64_t out_pitch, uint32_t flags, int32_t* d_status);

/* ---- tiled images: alpha ----
 * Byte +3 of an RGBA image, as a packed batch of its own over the same grid
 * (nx, ny, clamp padding): d_apacked, aoff[n + 1], alen[n] exactly as a packed
 * batch is defined above, plus akind[n] and aval[n] (u8).  The colour batch
 * and every call above are untouched.  Tile t's alpha plane A[y][x] is
 * tile_w x tile_h bytes, byte +3 of the padded tile, stored as one of
 *   kind 2, constant: every byte of the plane equals aval[t]; alen[t] = 0.
 *           Every tile of an opaque image is this kind.
 *   kind 0, coded: an ordinary NICE stream of the plane's triplet image,
 *           aw = ceil(tile_w / 3) wide, tile_h high, 3 channels, whose pixel
 *           (x', y) is (A[y][min(3x', tile_w - 1)], A[y][min(3x' + 1, tile_w - 1)],
 *           A[y][min(3x' + 2, tile_w - 1)]): byte for byte what nice_encode
 *           gives for that image with channels = channels_out = 3.
 *   kind 1, raw: the plane, tile_w * tile_h bytes in row-major order, where
 *           the verify decode (tolerant header) of the coded stream fails or
 *           differs, or the stream is not shorter than the plane
 *           (alen >= tile_w * tile_h; noise does this).
 * aval[t] is 0 unless the kind is 2. */
/* aw = ceil(tile_w / 3). */
uint32_t nice_tile_alpha_width(uint32_t tile_w);
/* n * align16(max(nice_encode_bound(aw, tile_h), tile_w * tile_h)): always
 * enough for d_apacked.  0 for a bad geometry. */
uint64_t nice_tiled_alpha_bound(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h);
/* The range pass alone: d_lo[t], d_hi[t] (n u32 each, device memory) = the
 * smallest and the largest byte +3 of tile t of a 4-channel image (padding
 * included: it repeats pixels of the same tile).  Asynchronous. */
int nice_tiles_alpha_range_dev(nice_ctx* ctx, void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w,
                               uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t* d_lo, uint32_t* d_hi);
/* Encodes the alpha batch of a 4-channel image (d_img, row_pitch >= 4 * w,
 * any alignment), read in place with the clamp padding.  d_apacked: 16-byte
 * aligned, apacked_cap bytes.  d_aoff (n + 1 u64) and *d_status are written as
 * by nice_encode_batch_packed_dev (NICE_E_CAPACITY: d_aoff[n] is the size
 * needed and no byte at or past apacked_cap is written); d_alen (n u64),
 * d_akind and d_aval (n u8); all device memory.
 * The call waits for the device at most twice: for the per-tile alpha ranges
 * (16 bytes per lane where d_img and row_pitch are 16-byte aligned, else
 * dwords or bytes), which decide which tiles are coded at all, and, only if
 * some tile is not constant, for the stream lengths that size the verify
 * decode.  Only the non-constant tiles are gathered, encoded and verified: an
 * opaque image costs the range pass and launches no encode and no decode.
 * Scratch is the context's, shared with nice_encode_tiled_dev. */
int nice_encode_tiled_alpha_dev(nice_ctx* ctx, void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w,
                                uint32_t h, uint32_t tile_w, uint32_t tile_h, uint8_t* d_apacked, uint64_t apacked_cap,
                                uint64_t* d_aoff /* n + 1 */, uint64_t* d_alen /* n */, uint8_t* d_akind /* n */,
                                uint8_t* d_aval /* n */, int32_t* d_status /* 1 */);
/* Writes byte +3, and only byte +3, of the 4-byte pixels of the window
 * [x0, x0 + rw) x [y0, y0 + rh) at d_out (out_pitch >= 4 * rw): run
 * nice_decode_tiled_dev with out_channels = 4 first, on the same stream, then
 * this.  h_aoff (n entries needed), h_alen, h_akind, h_aval: the tables of all
 * n tiles in host memory; only the tiles the rectangle touches are read
 * (d_apacked may be null when apacked_bytes is 0).  Nothing outside the window
 * is written.  Where tile_w % 4 == 0, x0 % 4 == 0 and d_out and out_pitch are
 * 16-byte aligned a lane rewrites the alpha of four pixels as one 16-byte
 * read-modify-write; everything else stores bytes.
 * d_status: one entry per selected tile, in the order of nice_decode_tiled_dev.
 * A tile whose status is not NICE_OK leaves its alpha bytes as they were; the
 * others are written.  Per tile: a kind above 2 is NICE_E_FORMAT; an offset
 * that is not a multiple of 16 or off + len > apacked_bytes NICE_E_ARG; a raw
 * length other than tile_w * tile_h, a constant tile with a nonzero length or
 * an empty stream NICE_E_FORMAT; a coded tile reports its decode status.
 * The call uploads the gathered tables and otherwise only enqueues work. */
int nice_decode_tiled_alpha_dev(nice_ctx* ctx, void* stream, const uint8_t* d_apacked, uint64_t apacked_bytes,
                                const uint64_t* h_aoff, const uint64_t* h_alen, const uint8_t* h_akind,
                                const uint8_t* h_aval, uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h,
                                uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh, uint8_t* d_out, uint64_t out_pitch,
                                int32_t* d_status);

/* ---- image sets ----
 * K >= 1 images of different sizes as one packed batch of tiles: a dataset or
 * a loader's minibatch is encoded, verified and decoded by one call of the
 * batch encoder and decoder, and a batch of M windows from M images decodes
 * only the tiles the windows touch.
 *
 * Image i is w[i] x h[i]; all images share `channels` (3 or 4) and one tile
 * size tile_w x tile_h, and each obeys the rules of nice_tile_grid, which
 * gives its nx[i] x ny[i] tiles.
 *   first[0] = 0, first[i + 1] = first[i] + nx[i] * ny[i], n = first[K]
 *   global tile first[i] + ty * nx[i] + tx is tile (tx, ty) of image i, padded
 *   by the clamp rule inside its own image
 * The set is one packed batch of n tiles: d_packed, off[n + 1], len[n],
 * kind[n], exactly as for a tiled image.  Tile first[i] + t of the set is,
 * byte for byte and kind for kind, tile t of nice_encode_tiled_dev of image i
 * alone at the same tile size: a set of one image is that image's tiled form,
 * and the tables of any set are its images' tables one after the other with
 * the offsets rebased.
 * NICE_E_ARG: K == 0, an image outside nice_tile_grid's limits, n times the
 * 1024-pixel encoder tiles of one tile >= 2^32, a launch grid that does not
 * fit.  The calls of this section do not store alpha: a 4-channel output gets
 * NICE_DEC_ALPHA_FILL_FF or 0 in byte +3, as a tiled image without an alpha
 * batch does.  The alpha batch of a set is a second packed batch with calls of
 * its own: "image sets: alpha" below.
 *
 * Host tables are parallel arrays: h_w, h_h (K u32), pointers and pitches (K
 * or M entries).  A window is five u32 {image, x0, y0, rw, rh}: the rectangle
 * [x0, x0 + rw) x [y0, y0 + rh) of image `image`; h_win holds M of them.  Its
 * slots are the tiles nice_tile_select gives inside its image, row-major; the
 * slots of window j are [slot_first[j], slot_first[j + 1]).  A tile that two
 * windows touch is one slot in each. */
/* Validates the set; first (K + 1 u32) receives the tile scan. */
int nice_set_grid(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                  uint32_t* first /* K + 1 */);
/* nice_packed_bound(n, tile_w, tile_h); 0 for a bad set. */
uint64_t nice_set_bound(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h);
/* slot_first (M + 1 u32): the exclusive scan of the windows' slot counts.
 * NICE_E_ARG: a bad set, M == 0, an image index >= K, an empty window or one
 * that leaves its image, 2^32 slots or more. */
int nice_set_select(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                    const uint32_t* h_win /* 5 * M */, uint32_t M, uint32_t* slot_first /* M + 1 */);
/* Images -> tiles.  Image i: rows of h_w[i] pixels, row y at h_img[i] +
 * y * h_pitch[i] (device memory; h_pitch[i] >= h_w[i] * channels; any
 * alignment).  Global tile g is written dense at d_tiles + g * tile_stride
 * (tile_stride >= tile_w * tile_h * channels) with the clamp padding.  One
 * launch whatever K is; each image moves as nice_tiles_split_dev would move it
 * (16 bytes per lane, dwords or bytes by its own alignment).  Asynchronous
 * after the upload of the K image descriptors. */
int nice_set_split_dev(nice_ctx* ctx, void* stream, const uint8_t* const* h_img, const uint64_t* h_pitch,
                       const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint8_t channels, uint32_t tile_w,
                       uint32_t tile_h, uint8_t* d_tiles, uint64_t tile_stride);
/* Slots -> windows.  Slot i (d_tiles + i * tile_stride, or, with d_src_off
 * non-null, d_tiles + d_src_off[i]: raw tiles straight from a packed buffer,
 * tile_channels must be 3) holds tile d_slot_tile[i], counted inside its
 * image, for window d_slot_win[i]; both tables are device memory, slots in any
 * order.  Skipped: a slot whose d_slot_status[i] (optional, device) is not 0,
 * a window index >= M, a tile index outside its image.  Window j goes to
 * h_out[j] (device memory) with row pitch h_out_pitch[j] >= rw * out_channels,
 * as nice_tiles_merge_dev writes its window: nothing outside a window is
 * written, and no padding.  The windows' outputs must not overlap.
 * tile_channels 3 -> out_channels 4 writes `alpha` as byte +3; 4 -> 3 drops
 * it.  One launch whatever M is; each window moves by its own alignment and
 * x0 % 4.  Asynchronous after the upload of the M window descriptors. */
int nice_set_merge_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                       const uint64_t* d_src_off, const uint32_t* d_slot_win, const uint32_t* d_slot_tile,
                       const int32_t* d_slot_status, uint32_t n_slots, uint8_t tile_channels, const uint32_t* h_w,
                       const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h, const uint32_t* h_win,
                       uint8_t* const* h_out, const uint64_t* h_out_pitch, uint32_t M, uint8_t out_channels,
                       uint8_t alpha);
/* Encodes K device-resident images as the n tiles of a set: the set split,
 * then exactly nice_encode_tiled_dev's sequence over all n tiles at once
 * (nice_encode_batch_dev, the verify decode with NICE_DEC_TOLERANT_HEADER, the
 * compare, the raw store, the pack).  The number of launches does not depend
 * on K.  d_packed, packed_cap (nice_set_bound() always suffices), d_off
 * (n + 1), d_len, d_kind (n), *d_status, the one wait and the scratch: as for
 * nice_encode_tiled_dev. */
int nice_encode_set_dev(nice_ctx* ctx, void* stream, const uint8_t* const* h_img, const uint64_t* h_pitch,
                        const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint8_t channels, uint8_t channels_out,
                        uint32_t tile_w, uint32_t tile_h, uint8_t* d_packed, uint64_t packed_cap,
                        uint64_t* d_off /* n + 1 */, uint64_t* d_len /* n */, uint8_t* d_kind /* n */,
                        int32_t* d_status /* 1 */);
/* Decodes M windows of a set, window j into h_out[j] (device memory, row
 * pitch h_out_pitch[j] >= rw * out_channels; the windows' outputs must not
 * overlap).  h_off, h_len, h_kind: the tables of all n tiles in host memory.
 * Every slot (above) is decoded on its own: a tile that two windows touch is
 * decoded once for each.  One batch decode over all coded slots, one status
 * scatter, one merge of the coded and one of the raw slots: the number of
 * launches does not depend on K or M.  Flags as for nice_decode_tiled_dev
 * (NICE_DEC_STRICT_REFERENCE is NICE_E_ARG).
 * d_status: slot_first[M] entries, one per slot, with nice_decode_tiled_dev's
 * codes; a slot whose status is not NICE_OK leaves its pixels untouched, the
 * others are written.  The call uploads the gathered tables and the window
 * descriptors and otherwise only enqueues work. */
int nice_decode_set_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                        const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind, const uint32_t* h_w,
                        const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h, const uint32_t* h_win,
                        uint8_t* const* h_out, const uint64_t* h_out_pitch, uint32_t M, uint8_t out_channels,
                        uint32_t flags, int32_t* d_status /* slot_first[M] */);

/* ---- image sets: alpha ----
 * Byte +3 of the K RGBA images of a set, as a packed batch of its own over the
 * same n global tiles: d_apacked, aoff[n + 1], alen[n], akind[n], aval[n],
 * laid out and with the kinds and the two raw rules exactly as "tiled images:
 * alpha" defines them.  Global tile first[i] + t equals tile t of
 * nice_encode_tiled_alpha_dev of image i alone in kind, value, stored bytes and
 * zero padding up to the next multiple of 16: a set of one image is that
 * image's tiled alpha batch, and the alpha tables of any set are its images'
 * alpha tables one after the other with the offsets rebased.  The colour batch
 * of the set and every call above are untouched. */
/* n * align16(max(nice_encode_bound(aw, tile_h), tile_w * tile_h)): always
 * enough for d_apacked.  0 for a bad set. */
uint64_t nice_set_alpha_bound(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h);
/* The range pass alone: d_lo[g], d_hi[g] (n u32 each, device memory) = the
 * smallest and the largest byte +3 of global tile g.  Images as for
 * nice_set_split_dev with channels = 4.  One launch whatever K is; each image
 * is read by its own alignment (16 bytes per lane, dwords or bytes).
 * Asynchronous after the upload of the K image descriptors. */
int nice_set_alpha_range_dev(nice_ctx* ctx, void* stream, const uint8_t* const* h_img, const uint64_t* h_pitch,
                             const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                             uint32_t* d_lo /* n */, uint32_t* d_hi /* n */);
/* Encodes the alpha batch of K device-resident 4-channel images (h_pitch[i] >=
 * 4 * h_w[i], any alignment), read in place.  The sequence is
 * nice_encode_tiled_alpha_dev's over all n tiles at once: the set range pass,
 * the first wait, the host verdict constant / not and the list of the m
 * non-constant global tiles, the set gather, nice_encode_batch_dev over the m
 * triplet images, the second wait, the tolerant verify decode, the compare,
 * verdict and raw store, the offset scan over the n lengths, the pack.  The
 * call waits at most twice and its number of launches does not depend on K; a
 * set whose images are all opaque launches no encode and no decode.
 * d_apacked, apacked_cap (nice_set_alpha_bound() always suffices), d_aoff,
 * d_alen, d_akind, d_aval, *d_status (NICE_E_CAPACITY included) and the
 * scratch: as for nice_encode_tiled_alpha_dev. */
int nice_encode_set_alpha_dev(nice_ctx* ctx, void* stream, const uint8_t* const* h_img, const uint64_t* h_pitch,
                              const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                              uint8_t* d_apacked, uint64_t apacked_cap, uint64_t* d_aoff /* n + 1 */,
                              uint64_t* d_alen /* n */, uint8_t* d_akind /* n */, uint8_t* d_aval /* n */,
                              int32_t* d_status /* 1 */);
/* Writes byte +3, and only byte +3, of the 4-byte pixels of M windows: run
 * nice_decode_set_dev with out_channels = 4 first, on the same stream and with
 * the same windows and outputs, then this.  h_aoff, h_alen, h_akind, h_aval:
 * the tables of all n tiles in host memory (d_apacked may be null when
 * apacked_bytes is 0).  Slots and their order are nice_set_select's; a tile
 * that two windows touch is one slot in each.  d_status: slot_first[M]
 * entries, with nice_decode_tiled_alpha_dev's host checks and codes per slot;
 * a coded slot reports its decode status.  A slot whose status is not NICE_OK
 * leaves its alpha bytes as the colour pass left them; the others are written.
 * Nothing outside a window is written.  A window whose base and pitch are
 * 16-byte aligned and whose x0 % 4 == 0 is written, where tile_w % 4 == 0, by
 * 16-byte read-modify-writes of four pixels; every other window by bytes, in
 * the same launch.  One upload (window descriptors and gathered tables), one
 * batch decode over the coded slots, one status scatter, one merge launch: the
 * number of launches depends on neither K nor M. */
int nice_decode_set_alpha_dev(nice_ctx* ctx, void* stream, const uint8_t* d_apacked, uint64_t apacked_bytes,
                              const uint64_t* h_aoff, const uint64_t* h_alen, const uint8_t* h_akind,
                              const uint8_t* h_aval, const uint32_t* h_w, const uint32_t* h_h, uint32_t K,
                              uint32_t tile_w, uint32_t tile_h, const uint32_t* h_win, uint8_t* const* h_out,
                              const uint64_t* h_out_pitch, uint32_t M, int32_t* d_status /* slot_first[M] */);

/* ---- image sets: tensor output ----
 * The windows of a set decoded straight into what a model reads: three
 * channels of float32, float16 or bfloat16, scaled and shifted per channel,
 * planar (NCHW) or interleaved (NHWC), each window optionally mirrored.  The
 * set merge converts as it stores; there is no uint8 intermediate.
 *
 * The value: for output channel c in {0, 1, 2} (bytes +0..+2 of the decoded
 * pixel) and byte value b,
 *   v = fmaf((float)b, scale[c], bias[c])       binary32, one rounding
 * NICE_TENSOR_F32 stores v; NICE_TENSOR_F16 and NICE_TENSOR_BF16 store v
 * converted round-to-nearest-even.  The result does not depend on the store
 * width, the layout, the flip or the kind of a tile.
 *
 * The output has three channels, always: a 4-channel set decodes its colour.
 * This path emits colour only; the alpha batch of a set ("image sets: alpha")
 * is neither read nor written by it.
 *
 * Window j is rw x rh elements per channel at h_out[j] (device memory, aligned
 * to the element size), pitches counted in elements:
 *   NICE_TENSOR_PLANAR       (c, y, x) at h_out[j] + c * h_plane_pitch[j] + y * h_row_pitch[j] + x
 *                            (h_row_pitch[j] >= rw)
 *   NICE_TENSOR_INTERLEAVED  (c, y, x) at h_out[j] + y * h_row_pitch[j] + 3 * x + c
 *                            (h_row_pitch[j] >= 3 * rw; h_plane_pitch is not read)
 * h_flip (M bytes, or null: none): h_flip[j] != 0 mirrors window j, output
 * column x takes image column x0 + rw - 1 - x.  The windows' outputs must not
 * overlap; nothing outside a window's elements is written, and no padding.
 * NICE_E_ARG besides the errors of the uint8 calls: an unknown dtype or
 * layout, a base pointer not aligned to the element size, a row pitch below
 * the window, scale or bias null or not finite. */
#define NICE_TENSOR_F32  0u
#define NICE_TENSOR_F16  1u
#define NICE_TENSOR_BF16 2u
#define NICE_TENSOR_PLANAR      0u
#define NICE_TENSOR_INTERLEAVED 1u
/* The kernel alone, as nice_set_merge_dev is for the uint8 merge: the same
 * slots (d_tiles, tile_stride, d_src_off, the slot tables, tile_channels 3 or
 * 4; byte +3 of a 4-byte slot pixel is ignored), the same skips, one launch
 * whatever M is.  Dense 4-byte slots at 4-byte alignment are read as dwords;
 * a lane converts 1, 2, 4 or 8 consecutive pixels and stores them per plane as
 * one store of up to 16 bytes, as far as the window's base, its pitches, x0
 * (mirrored: x0 + rw) and the slots' alignment and tile_w allow; every other
 * window goes element by element, in the same launch.  Asynchronous after the
 * upload of the M window descriptors. */
int nice_set_merge_tensor_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                              const uint64_t* d_src_off, const uint32_t* d_slot_win, const uint32_t* d_slot_tile,
                              const int32_t* d_slot_status, uint32_t n_slots, uint8_t tile_channels /* 3 or 4 */,
                              const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                              const uint32_t* h_win, const uint8_t* h_flip /* M, or null */, void* const* h_out,
                              const uint64_t* h_row_pitch, const uint64_t* h_plane_pitch /* planar only */, uint32_t M,
                              uint32_t dtype, uint32_t layout, const float* scale /* 3 */, const float* bias /* 3 */);
/* nice_decode_set_dev with the tensor merge in place of both merges: the same
 * tables, slots, per-slot statuses and their order, host-side checks of raw
 * slots and errors.  The coded slots are decoded at 4 bytes per pixel whatever
 * the set's channel count; raw slots are read in place, 3 bytes per pixel.  One
 * upload, one batch decode over the coded slots, one status scatter, one
 * tensor merge of the coded and one of the raw slots: the number of launches
 * depends on neither K nor M.  A slot whose status is not NICE_OK leaves its
 * elements untouched.  NICE_DEC_ALPHA_FILL_FF is accepted and irrelevant;
 * NICE_DEC_STRICT_REFERENCE is NICE_E_ARG. */
int nice_decode_set_tensor_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                               const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind,
                               const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                               const uint32_t* h_win, const uint8_t* h_flip, void* const* h_out,
                               const uint64_t* h_row_pitch, const uint64_t* h_plane_pitch, uint32_t M,
                               uint32_t dtype, uint32_t layout, const float* scale, const float* bias,
                               uint32_t flags, int32_t* d_status /* slot_first[M] */);

/* ---- image sets: resized tensor output ----
 * "image sets: tensor output" with every window resampled to one size,
 * out_h x out_w, whatever its own: the random resized crop of a training
 * loader, from the packed set to [M, 3, out_h, out_w] in one call.  Dtypes,
 * layouts, pitches, h_flip, scale and bias are the tensor output's; window j
 * is out_w x out_h elements per channel at h_out[j] (h_row_pitch[j] >= out_w,
 * interleaved >= 3 * out_w).
 *
 * The value is defined exactly, so results compare bit for bit: fixed-point
 * bilinear sampling with 8 fractional bits of position and no antialiasing (a
 * strong reduction aliases, as torch's antialias=False does).  For an output
 * axis of n_out elements over a window axis of n_in pixels the position of
 * output index x is the integer q, in 1/256 of a pixel (64-bit unsigned
 * arithmetic, floor division; the subtraction stops at 0):
 *   t  = ((2x + 1) * n_in * 256 + n_out) / (2 * n_out)   nearest 1/256 to (x + 1/2) * n_in / n_out, halves up
 *   q  = clamp(t - 128, 0, (n_in - 1) * 256)             minus the half pixel
 *   i0 = q >> 8,  f = q & 255,  i1 = min(i0 + (f != 0), n_in - 1)
 * Indices are relative to the window and the clamp is to the window, not the
 * image: a resized window reads no pixel outside itself and touches exactly
 * the tiles nice_set_select reports for it.  A mirrored window computes the
 * column position from out_w - 1 - x.  With (i0, i1, fx) for the column,
 * (j0, j1, fy) for the row and b the byte of channel c,
 *   acc = (256 - fy) * ((256 - fx) * b[j0][i0] + fx * b[j0][i1])
 *       +        fy  * ((256 - fx) * b[j1][i0] + fx * b[j1][i1])
 *   v   = fmaf((float)acc * 0x1p-16f, scale[c], bias[c])
 * acc <= 255 * 65536 < 2^24, so the conversion and the scaling by 2^-16 are
 * exact and the fmaf is the one rounding.  NICE_TENSOR_F32 stores v, the
 * 16-bit types v rounded to nearest even.  Where out_w == rw and out_h == rh,
 * f is 0 everywhere, acc = b << 16, and the result is the tensor output's bit
 * for bit; an exact halving of both axes gives the mean of each 2 x 2 block.
 *
 * An element is written iff every slot one of its taps falls in has status
 * NICE_OK and a readable source (a tap of weight 0 coincides with its
 * neighbour, so an element of an unresized window depends on one slot); else
 * it is left untouched.  Nothing outside a window's 3 * out_h * out_w elements
 * is written.  NICE_E_ARG besides the errors of the tensor calls: out_w or
 * out_h 0 or above NICE_RESIZE_MAX. */
#define NICE_RESIZE_MAX 8192u
/* the kinds of d_src, its bits 62-63 */
#define NICE_SRC_DENSE 0u
#define NICE_SRC_RAW   1u
#define NICE_SRC_NONE  3u
/* The kernel alone.  d_src: slot_first[M] u64 in device memory, one per slot
 * in nice_set_select's order, saying where the slot's pixels are:
 *   bits 62-63  0 dense, 4 bytes per pixel (byte +3 ignored) at d_tiles + value * tile_stride
 *                 (d_tiles and tile_stride multiples of 4: a tap is one dword load)
 *               1 raw, 3 bytes per pixel at d_packed + value
 *               3 nothing to read (2 is read as 3)
 *   bits 0-61   value
 * d_slot_status: slot_first[M] codes, or null (all NICE_OK).  Dense or raw is
 * decided per tap by d_src, so there is one launch whatever M is and whatever
 * the slots are.  A lane owns 1, 2 or 4 consecutive output columns, whose
 * positions it computes once per block, and stores them per plane as one store
 * of 4, 8 or 16 bytes as far as the window's base and pitches allow; every
 * other window goes element by element, in the same launch.  Asynchronous after the
 * upload of the M window descriptors. */
int nice_set_resize_tensor_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                               const uint8_t* d_packed, const uint64_t* d_src /* slot_first[M] */,
                               const int32_t* d_slot_status /* slot_first[M], or null */, const uint32_t* h_w,
                               const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                               const uint32_t* h_win, const uint8_t* h_flip /* M, or null */, uint32_t out_w,
                               uint32_t out_h, void* const* h_out, const uint64_t* h_row_pitch,
                               const uint64_t* h_plane_pitch /* planar only */, uint32_t M, uint32_t dtype,
                               uint32_t layout, const float* scale /* 3 */, const float* bias /* 3 */);
/* nice_decode_set_tensor_dev with out_w, out_h and the one resize launch in
 * place of the two tensor merges: the same host tables, slots, per-slot
 * statuses and their order, host-side refusals and flags; coded slots decoded
 * at 4 bytes per pixel, raw slots read in place.  One upload (the position
 * column d_src travels behind the window descriptors), one batch decode over
 * the coded slots, one status scatter, one resize launch: the number of
 * launches depends on neither K nor M. */
int nice_decode_set_resized_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                                const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind,
                                const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                                const uint32_t* h_win, const uint8_t* h_flip, uint32_t out_w, uint32_t out_h,
                                void* const* h_out, const uint64_t* h_row_pitch, const uint64_t* h_plane_pitch,
                                uint32_t M, uint32_t dtype, uint32_t layout, const float* scale, const float* bias,
                                uint32_t flags, int32_t* d_status /* slot_first[M] */);

/* ---- image sets: antialiased resized tensor output ----
 * The resized tensor output above with a reducing axis filtered, not sampled:
 * the triangle filter of support n_in / n_out that torch's
 * interpolate(bilinear, antialias=True) and PIL's resize apply, in integers, so
 * results compare bit for bit.  Windows, slots, d_src, dtypes, layouts,
 * pitches, h_flip, scale, bias, statuses, refusals and flags are the resized
 * tensor output's; only the value differs.  Each axis is treated separately.
 *
 * A non-reducing axis (n_out >= n_in): the taps (i0, i1, f) of the position
 * above, with the weights 16 * (256 - f) on i0 and 16 * f on i1, in 1/4096
 * (one tap where f == 0).
 *
 * A reducing axis (n_out < n_in; n_in <= NICE_RESIZE_AA_MAX_IN, else
 * NICE_E_ARG): for output index x (a mirrored window takes out_w - 1 - x on
 * the column axis) let
 *   C = (2x + 1) * n_in,  P_i = (2i + 1) * n_out,  S = 2 * n_in     (below 2^30)
 *   r_i = S - |P_i - C|   for 0 <= i < n_in      the raw weight of pixel i
 * The taps are the i with r_i > 0: one contiguous run lo..hi, relative to the
 * window and inside it (the window is never left).  With R the sum of all r_i
 * of the run and cum_i = r_lo + ... + r_i (64-bit, floor division),
 *   W_i = (cum * 8192 + R) / (2 * R)      with cum = cum_i;  W_(lo-1) = 0
 *   w_i = W_i - W_(i-1)
 * The w_i are not negative, sum to 4096 exactly, and each is within 1/4096 of
 * r_i / R; renormalising at a window edge is the same rule.  There is no limit
 * on the reduction ratio.
 *
 * The element: with column taps (i, w_i), row taps (j, v_j) and b the byte of
 * channel c,
 *   h[j]  = sum over i of w_i * b[j][i]             at most 255 * 2^12
 *   acc32 = sum over j of v_j * h[j]                at most 255 * 2^24
 *   acc   = (acc32 + 128) >> 8                      at most 255 * 65536
 *   v     = fmaf((float)acc * 0x1p-16f, scale[c], bias[c])
 * stored as the other tensor outputs store v.  A window that reduces on
 * neither axis has acc32 = 256 * (the acc above) and gives the resized tensor
 * output's bits; a window of the output's size gives the tensor output's; an
 * exact halving has the interior weights 512, 1536, 1536, 512 (the triangle of
 * support 2, not the 2 x 2 block mean).
 *
 * An element is written iff every slot its tap rectangle meets (columns
 * lo..hi by rows lo..hi; i0..i1 on a non-reducing axis) has status NICE_OK and
 * a readable source; else it is left untouched.  Nothing outside a window's
 * 3 * out_h * out_w elements is written. */
#define NICE_RESIZE_AA_MAX_IN 65536u
/* The kernels alone: nice_set_resize_tensor_dev's parameters.  Two launches
 * whatever M is and whatever the slots are: the weights of every reducing axis
 * into a table in the context's scratch (computed on the device, one thread
 * per source pixel), then the filter.  The filter is separable: a block walks
 * the source rows of a band of output rows once, stages each row's span in LDS
 * (the slot of a pixel is looked up once, not once per tap), sums the column
 * taps per lane and adds the row sums into the band's accumulators; the work
 * per window is proportional to its pixels, and no tap count is bounded.
 * A lane owns one output column: planar elements go one per plane and lane
 * (consecutive lanes, consecutive elements), an interleaved float32 pixel as
 * one 12-byte store, an interleaved 16-bit pixel as three stores.
 * Asynchronous after the upload of the M window descriptors. */
int nice_set_resize_aa_tensor_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                                  const uint8_t* d_packed, const uint64_t* d_src /* slot_first[M] */,
                                  const int32_t* d_slot_status /* slot_first[M], or null */, const uint32_t* h_w,
                                  const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                                  const uint32_t* h_win, const uint8_t* h_flip /* M, or null */, uint32_t out_w,
                                  uint32_t out_h, void* const* h_out, const uint64_t* h_row_pitch,
                                  const uint64_t* h_plane_pitch /* planar only */, uint32_t M, uint32_t dtype,
                                  uint32_t layout, const float* scale /* 3 */, const float* bias /* 3 */);
/* nice_decode_set_resized_dev with the antialiased value: the same host
 * tables, slots, per-slot statuses and their order, host-side refusals and
 * flags.  One upload, one batch decode over the coded slots, one status
 * scatter, then the two resample launches: the number of launches depends on
 * neither K nor M. */
int nice_decode_set_resized_aa_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                                   const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind,
                                   const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w,
                                   uint32_t tile_h, const uint32_t* h_win, const uint8_t* h_flip, uint32_t out_w,
                                   uint32_t out_h, void* const* h_out, const uint64_t* h_row_pitch,
                                   const uint64_t* h_plane_pitch, uint32_t M, uint32_t dtype, uint32_t layout,
                                   const float* scale, const float* bias, uint32_t flags,
                                   int32_t* d_status /* slot_first[M] */);

/* ---- one image sharded over ranks (config 4) ----
 * The image's raster is cut into bands of whole encoder tiles (1024 pixels in
 * raster order); rank r encodes tiles [tile_lo, tile_hi).  The caller runs the
 * exchange steps between the calls (bench/tests use RCCL via torch.distributed):
 *   1. nice_band_classify   band records + d_edges = {first, last} coded pixel
 *                           (0xFFFFFFFF: none)
 *   2. all-gather edges     band_next = first coded pixel of the later bands (w*h: none)
 *      nice_band_runs       the band's symbol histogram (858 x u32) into d_hist
 *   3. all-reduce (sum)     nice_band_tables: identical code tables on every rank;
 *                           returns the band's data bits and the data start bit
 *   4. all-gather bits      band_bit0 = data start + bits of the earlier bands
 *      nice_band_pack       nice_band_words() words: the band's bits at their
 *                           stream position (first/last word partial)
 *   5. gather words         nice_band_assemble (one rank): header + bands + tail
 * The result equals nice_encode of the whole image byte for byte, codes longer
 * than 25 bits included.  nice_band_words() counts the band's stream words plus
 * a two-word trailer (every band has one, a band of 0 bits only the trailer):
 * a code longer than 25 bits that starts in the byte holding band_bit0
 * rewrites (reference writer wrap, bitwriter.rs:55-73) bits of the previous
 * band; it is recorded there and applied by nice_band_assemble.
 * Device-resident variants (no host synchronisation between the steps; the
 * exchanges can stay on device, e.g. RCCL collectives on the same stream):
 *   nice_band_runs_dev      band_next read from device memory (u32)
 *   nice_band_tables_dev    d_info[0] = the band's data bits, d_info[1] = the
 *                           data start bit (device u64 x 2, written in stream
 *                           order; the context keeps its own copy, so d_info may
 *                           be freed or reused once the call's work has run)
 *   nice_band_pack_bits     the band's bits passed in (from the gathered d_info);
 *                           band_bits must equal d_info[0] exactly (it sizes the
 *                           band's words): after nice_band_tables_dev the device
 *                           compares them and, on a mismatch, writes no band bits
 *                           (d_words never overrun) and marks the band's trailer;
 *                           nice_band_assemble then returns NICE_E_ARG
 * nice_band_assemble after nice_band_tables_dev takes band_bit0[0] as the data
 * start.
 * d_px holds pixels [px0, px0 + px_count) (global raster index), which must
 * cover the band and the 3 rows + 3 pixels before it. */
int nice_band_classify(nice_ctx* ctx, void* stream, const uint8_t* d_px, uint64_t px0, uint64_t px_count,
                       uint32_t w, uint32_t h, uint8_t channels, uint8_t channels_out, uint32_t tile_lo,
                       uint32_t tile_hi, uint32_t* d_edges);
int nice_band_runs(nice_ctx* ctx, void* stream, uint32_t band_next, uint32_t* d_hist);
int nice_band_tables(nice_ctx* ctx, void* stream, const uint32_t* d_hist_total, uint64_t* band_bits,
                     uint64_t* seed_bit);
int nice_band_runs_dev(nice_ctx* ctx, void* stream, const uint32_t* d_band_next, uint32_t* d_hist);
int nice_band_tables_dev(nice_ctx* ctx, void* stream, const uint32_t* d_hist_total, uint64_t* d_info);
uint64_t nice_band_words(uint64_t band_bit0, uint64_t band_bits);
int nice_band_pack(nice_ctx* ctx, void* stream, uint64_t band_bit0, uint32_t* d_words, uint64_t words_cap);
int nice_band_pack_bits(nice_ctx* ctx, void* stream, uint64_t band_bit0, uint64_t band_bits, uint32_t* d_words,
                        uint64_t words_cap);
int nice_band_assemble(nice_ctx* ctx, void* stream, const uint32_t* d_words, const uint64_t* band_bit0,
                       const uint64_t* band_bits, uint32_t n_bands, uint8_t* d_out, uint64_t out_cap,
                       uint64_t* out_len);
/* Encoder tile size (pixels) used by the band API. */
uint32_t nice_tile_pixels(void);

/* ---- streamed host pipeline (BASELINE config 5) ----
 * Frames in host memory flow through `depth` slots of `batch` frames; each slot
 * has its own HIP stream, scratch and device buffers, so one slot's H2D copy,
 * another's kernels and a third's D2H copy overlap.  Replaces calling
 * code::encode / code::decode (code.rs:59-64, 464-468) once per image from host
 * memory (main.rs:28-103).  Host buffers may be pinned (copies asynchronous) or
 * pageable.  Frames are w x h with `channels` bytes per pixel (fixed per pipe). */
typedef struct nice_pipe nice_pipe;
int nice_pipe_create(int device, uint32_t w, uint32_t h, uint8_t channels, uint32_t batch, uint32_t depth,
                     nice_pipe** out);
void nice_pipe_destroy(nice_pipe* p);
/* Bytes per stream slot on the device (>= nice_encode_bound(w, h)). */
uint64_t nice_pipe_stream_stride(const nice_pipe* p);
/* px[f]: frame f (w*h*channels bytes).  out[f]: stream f (out_cap bytes
 * available), out_len[f] its length.  Blocks until every stream is on the host. */
int nice_pipe_encode(nice_pipe* p, const uint8_t* const* px, uint32_t n_frames, uint8_t channels_out,
                     uint8_t* const* out, uint64_t out_cap, uint64_t* out_len);
/* streams[f], stream_len[f] -> px[f] (w*h*out_channels bytes, out_channels <=
 * the pipe's channels); status[f] per frame (flags as nice_decode).  Blocks.
 * px[f] is defined only where status[f] == NICE_OK. */
int nice_pipe_decode(nice_pipe* p, const uint8_t* const* streams, const uint64_t* stream_len, uint32_t n_frames,
                     uint8_t out_channels, uint8_t* const* px, uint32_t flags, int32_t* status);
/* Per-frame checksums computed on the device from what the pipe copies to the
 * host (end-to-end checks of streamed runs whose host buffers are reused):
 * while set, nice_pipe_encode writes enc_sums[f] = nice_checksum64 of stream f
 * and nice_pipe_decode dec_sums[f] = that of frame f's pixels (either pointer
 * may be null; each must hold n_frames entries of the calls that follow).
 * nice_checksum64 of n bytes: zero-pad to whole little-endian u32 words w_i,
 * A = sum w_i, B = sum (i + 1) w_i (mod 2^64), checksum = A + 0x9E3779B97F4A7C15 B
 * (mod 2^64). */
int nice_pipe_set_checksums(nice_pipe* p, uint64_t* enc_sums, uint64_t* dec_sums);

/* ---- command-line front end helper (host only) ----
 * Reverses the PNG scanline filters (types 0-4) of h rows of w pixels of bpp
 * bytes: raw = h x (1 filter byte + w*bpp bytes), out = h x w*bpp bytes.  The
 * reference CLI (main.rs:28-133) reads and writes PNG with the png crate. */
int nice_png_unfilter(const uint8_t* raw, uint32_t w, uint32_t h, uint32_t bpp, uint8_t* out);

/* ---- 5x5 sub-block traversal ----
 * d_pos[i] = Image::new(w, h, _).calc_pos_from(index0 + i) for i < count
 * (image.rs:45-102), computed on `device`, asynchronous on `stream`.  The
 * reference's map exactly: not a permutation when w % 5 and h % 5 are both
 * nonzero, and positions >= w*h for some shapes (w = 7, ...).  w == 0 is
 * NICE_E_ARG (the reference divides by zero).  The codec does not use it. */
int nice_subblock_positions_dev(int device, void* stream, uint32_t w, uint32_t h, uint64_t index0,
                                uint64_t count, uint64_t* d_pos);

/* ---- per-kernel timing (HIP events on the call's stream), for benchmarks ---- */
enum {
  NICE_PH_ENC_CLASSIFY = 0, NICE_PH_ENC_TAILRUNS, NICE_PH_ENC_TABLES, NICE_PH_ENC_HEADER,
  NICE_PH_ENC_TILEBITS, NICE_PH_ENC_TILESCAN, NICE_PH_ENC_PACK, NICE_PH_ENC_TAIL, NICE_PH_ENC_LONG,
  NICE_PH_DEC_TABLES, NICE_PH_DEC_SYNC, NICE_PH_DEC_SCAN, NICE_PH_DEC_EMIT, NICE_PH_DEC_RECON,
  NICE_PH_DEC_PLACE, NICE_PH_DEC_RESYNC, NICE_PHASES   /* RESYNC: sync iterations after the first */
};
int nice_ctx_set_timing(nice_ctx* ctx, int on);
/* Sums (ms) and launch counts per phase since the last read; synchronises. */
int nice_ctx_read_timing(nice_ctx* ctx, double* ms, uint32_t* count);
const char* nice_phase_name(int phase);

#ifdef __cplusplus
}
#endif
#endif /* NICE_H */
