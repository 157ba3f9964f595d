// Baseline JPEG entropy (Huffman) decoder: the host half of the GPU JPEG decode
// (--gpu_jpeg_decode). It turns a JPEG's entropy-coded scan into quantised DCT coefficients of the
// block window a crop needs; dequantisation, IDCT, chroma upsampling, colour conversion and the
// crop run on the GPU (csrc/kernels/jpeg.hip; definition: data/jpeg.py jpeg_decode_reference).
//
// Record written at dst (16-byte aligned), all little endian:
//   int32  header[32]                       (128 bytes, fields below)
//   uint16 qtables[4][64]                   (512 bytes, natural order; unused tables are zero)
//   int16  coefficients[nblocks][64]        (natural order after de-zigzag), component after
//                                           component, each component's window row-major in blocks
// Header fields: HDR_*. The window is MCU aligned and holds the crop plus, where the chroma planes
// are subsampled, one chroma sample of margin on each side (clipped to the image), which is what
// the triangle upsampling filter reads.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hcbjpeg {

constexpr int HDR_INTS = 32;
constexpr int32_t HDR_MAGIC = 0x3147504a;  // "JPG1"
enum {
  HDR_MAGIC_AT = 0,
  HDR_NCOMP = 1,   // 1 (grey) or 3 (YCbCr)
  HDR_HS = 2,      // luma sampling factors (1 | 2); chroma is 1x1
  HDR_VS = 3,
  HDR_H = 4,       // the image's true height and width
  HDR_W = 5,
  HDR_CY = 6,      // crop window in image pixels: y, x, h, w
  HDR_CX = 7,
  HDR_CH = 8,
  HDR_CW = 9,
  HDR_OY = 10,     // crop offset inside the luma window, pixels
  HDR_OX = 11,
  HDR_COMP = 12,   // per component c at HDR_COMP + 6 c: bx0, by0 (window origin in the component's
                   // block grid), bw, bh (extent in blocks), quantisation table, first block
  HDR_NBLOCKS = 30,
  HDR_BYTES = 31,  // size of the whole record
};
constexpr size_t QT_OFFSET = HDR_INTS * 4;
constexpr size_t COEF_OFFSET = QT_OFFSET + 4 * 64 * 2;

// Decodes data[0, n) for the crop window (y, x, h, w) in image pixels (h <= 0 or w <= 0: the whole
// image) into dst[0, cap). Returns the bytes written, or -1 with *reason set to a static string
// (the caller then decodes that image another way). Never reads outside data or writes outside dst.
long jpeg_entropy_decode(const uint8_t* data, size_t n, int wy, int wx, int wh, int ww, uint8_t* dst, size_t cap,
                         const char** reason);

}  // namespace hcbjpeg
