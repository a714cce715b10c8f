// mx_nlm_lut.h — the weight table of mx_denoise_nlm_u8 (include/mx_det.h): LUT[i] = round(4096 * exp(-i / 16))
// for i = 0..127, as literals; an index of 128 and above weighs 0. Nothing computes exp at run time; the numpy
// restatement (tests/denoise_ref.py) holds the same 128 integers and a test compares the two.
#pragma once

#define MX_NLM_LUT_SIZE 128
// clang-format off
#define MX_NLM_LUT_VALUES \
  4096, 3848, 3615, 3396, 3190, 2997, 2815, 2645, 2484, 2334, 2192, 2060, 1935, 1818, 1707, 1604, \
  1507, 1416, 1330, 1249, 1174, 1102, 1036, 973, 914, 859, 807, 758, 712, 669, 628, 590, \
  554, 521, 489, 460, 432, 406, 381, 358, 336, 316, 297, 279, 262, 246, 231, 217, \
  204, 192, 180, 169, 159, 149, 140, 132, 124, 116, 109, 103, 96, 90, 85, 80, \
  75, 70, 66, 62, 58, 55, 52, 48, 46, 43, 40, 38, 35, 33, 31, 29, \
  28, 26, 24, 23, 21, 20, 19, 18, 17, 16, 15, 14, 13, 12, 12, 11, \
  10, 10, 9, 8, 8, 7, 7, 7, 6, 6, 5, 5, 5, 5, 4, 4, \
  4, 4, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 1
// clang-format on
