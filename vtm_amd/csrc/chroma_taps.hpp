// chroma_taps.hpp -- H.266 table 28 (the 4-tap filter at 1/32 sample phases; InterpolationFilter::m_chromaFilter, CommonLib/InterpolationFilter.cpp:132-166) as the text
// of an initialiser, so the table is written once: mc_block.hpp fills its __constant__ array from it (4:2:0 chroma motion compensation), intra.hip fills the cubic
// taps of the fractional angular intra modes (IntraPrediction.cpp:576 takes them from the same table) and host/test_intra.cpp a host array.
#pragma once

#define VTMHIP_CHROMA_FILTER_TAPS                                                                                                                                 \
  { 0, 64, 0, 0 },    { -1, 63, 2, 0 },   { -2, 62, 4, 0 },   { -2, 60, 7, -1 },  { -2, 58, 10, -2 }, { -3, 57, 12, -2 }, { -4, 56, 14, -2 }, { -4, 55, 15, -2 }, \
  { -4, 54, 16, -2 }, { -5, 53, 18, -2 }, { -6, 52, 20, -2 }, { -6, 49, 24, -3 }, { -6, 46, 28, -4 }, { -5, 44, 29, -4 }, { -4, 42, 30, -4 }, { -4, 39, 33, -4 }, \
  { -4, 36, 36, -4 }, { -4, 33, 39, -4 }, { -4, 30, 42, -4 }, { -4, 29, 44, -5 }, { -4, 28, 46, -6 }, { -3, 24, 49, -6 }, { -2, 20, 52, -6 }, { -2, 18, 53, -5 }, \
  { -2, 16, 54, -4 }, { -2, 15, 55, -4 }, { -2, 14, 56, -4 }, { -2, 12, 57, -3 }, { -2, 10, 58, -2 }, { -1, 7, 60, -2 },  { 0, 4, 62, -2 },   { 0, 2, 63, -1 }
