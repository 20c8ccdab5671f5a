// fi_jpeg_view.h -- the view of a GPU JPEG decode (fi_jpeg_decode_device_view):
// an EXIF orientation applied to the decoded image and a rectangle of the
// oriented image.  One index map, shared by the host (validation, the
// stand-alone driver tests/native/jpeg_view_driver.cpp) and k_jpeg_color_view.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FI_VIEW_HD __host__ __device__ __forceinline__
#else
#define FI_VIEW_HD inline
#endif

namespace fi {

// Orientations 5..8 swap the axes: the oriented image of a W x H source is H x W.
FI_VIEW_HD bool jpeg_view_transposed(int o) { return o >= 5; }

// Source pixel (sx, sy) of pixel (u, v) of the oriented image, for EXIF
// orientation o (1..8) of a W x H source.  What Pillow's ImageOps.exif_transpose
// applies: 2 FLIP_LEFT_RIGHT, 3 ROTATE_180, 4 FLIP_TOP_BOTTOM, 5 TRANSPOSE,
// 6 ROTATE_270, 7 TRANSVERSE, 8 ROTATE_90.
FI_VIEW_HD void jpeg_view_map(int o, int W, int H, int u, int v, int *sx, int *sy) {
  const int a = o >= 5 ? v : u, b = o >= 5 ? u : v;  // along the source row / column before the flips
  const bool fx = o == 2 || o == 3 || o == 7 || o == 8;
  const bool fy = o == 3 || o == 4 || o == 6 || o == 7;
  *sx = fx ? W - 1 - a : a;
  *sy = fy ? H - 1 - b : b;
}

}  // namespace fi
