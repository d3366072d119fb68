// Global memory <-> the MFMA fragment layout, through a wave-private LDS block: the layout of `struct tile_io` in
// csrc/layer_tail_x6.hip.  That file keeps its own copy of the offsets: built on this header (make_tile_io around make_tile_xpose,
// store32 / load32_finish around tile_to_rows / tile_to_frag) its forward kernel compiles to 236 VGPRs instead of 238 and both tail
// kernels to a different instruction order (no scratch either way) - a change of the step's two largest kernels that would have
// to be measured on its own.
//
// In the fragment layout lane (c, g) = (lane % 16, lane / 16) holds columns 8 g .. 8 g + 7 of token c of a 16-token x 32-column
// fp32 block: consecutive lanes are consecutive ROWS, so a dwordx4 access of a wave touches 64 separate 16-byte pieces.  In the
// row layout lane l holds, in instruction i (0, 1), row 8 i + l / 8, columns 4 (l % 8) .. + 3: 8 consecutive lanes = one full
// 128-byte line.  The block (2 KiB) passes through LDS to change layout; the 16-byte slots of a row are XOR-swizzled with the
// row so that both sides are bank-conflict-free (ds_*_b128 lane groups).  One wave, in-order LDS: no barrier.
#pragma once

typedef float tio_f32x4 __attribute__((ext_vector_type(4)));

struct tile_xpose {
  unsigned char* scr;   // this wave's 2 KiB
  int frag_off0;        // fragment side: slot 2 g of row c (the second half: ^ 16)
  int row_off[2];       // row side, instruction i: row 8 i + lane / 8, slot lane % 8
};
__device__ __forceinline__ tile_xpose make_tile_xpose(unsigned char* scr, int lane) {
  tile_xpose t;
  const int c = lane & 15, g = lane >> 4, r = lane >> 3, p = lane & 7;
  t.scr = scr;
  t.frag_off0 = c * 128 + (((2 * g) ^ (c & 7)) << 4);
  t.row_off[0] = r * 128 + ((p ^ r) << 4);           // r < 8
  t.row_off[1] = t.row_off[0] + 8 * 128;             // row r + 8: the same slot
  return t;
}
// row layout (w0: row lane / 8, w1: row 8 + lane / 8) -> fragment layout (v0: columns 8 g .. + 3, v1: 8 g + 4 .. + 7 of token c)
__device__ __forceinline__ void tile_to_frag(const tile_xpose& t, const tio_f32x4& w0, const tio_f32x4& w1, tio_f32x4& v0,
                                             tio_f32x4& v1) {
  *(tio_f32x4*)(t.scr + t.row_off[0]) = w0;
  *(tio_f32x4*)(t.scr + t.row_off[1]) = w1;
  v0 = *(const tio_f32x4*)(t.scr + t.frag_off0);
  v1 = *(const tio_f32x4*)(t.scr + (t.frag_off0 ^ 16));
}
// fragment layout -> row layout
__device__ __forceinline__ void tile_to_rows(const tile_xpose& t, const tio_f32x4& v0, const tio_f32x4& v1, tio_f32x4& w0,
                                             tio_f32x4& w1) {
  *(tio_f32x4*)(t.scr + t.frag_off0) = v0;
  *(tio_f32x4*)(t.scr + (t.frag_off0 ^ 16)) = v1;
  w0 = *(const tio_f32x4*)(t.scr + t.row_off[0]);
  w1 = *(const tio_f32x4*)(t.scr + t.row_off[1]);
}
