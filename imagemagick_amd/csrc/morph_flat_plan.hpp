// Host plan of the flat Erode / Dilate kernels (morphology_flat.hip): a cell list as one run per kernel row, the
// distinct half-widths of the runs, and from them the level tables of morph_convex_kernel, the rectangle tables of
// morph_rects_kernel and whether the latter takes the shape at a given pixel size.  All of it depends on the kernel
// alone, so the route is known before anything is packed, padded, uploaded or launched.  Plain C++, no device code.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace mh {

struct Cell
{
  int dx,dy;       // offset of the sample inside the LDS tile, relative to the output pixel's tile position
  double value;
};

struct FlatShape
{
  int dy_min=0,dy_max=0,span=0;      // kernel rows dy_min .. dy_max, span of them
  int top=0,bottom=0;                // kernel rows above / below the output row
  int cx=0,hmax=0;                   // common centre column of the runs, widest half-width
  bool full=true;                    // no empty row between dy_min and dy_max
  std::vector<int> half;             // [span] row dy_min+k is the run [cx-half[k], cx+half[k]]; -1: an empty row
  std::vector<int> widths;           // the distinct half-widths, ascending: the levels of both kernels
};

// false when the active cells are not one gap-free run per row about one centre column (Ring, Cross, user
// kernels ...), or there are none
static inline bool flat_shape(const Cell *cells,size_t ncells,FlatShape &s)
{
  if (ncells == 0)
    return false;
  s=FlatShape();
  s.dy_min=s.dy_max=cells[0].dy;
  for (size_t i=0; i < ncells; i++)
    {
      s.dy_min=std::min(s.dy_min,cells[i].dy);
      s.dy_max=std::max(s.dy_max,cells[i].dy);
    }
  s.span=s.dy_max-s.dy_min+1;
  s.top=s.dy_min < 0 ? -s.dy_min : 0;
  s.bottom=s.dy_max > 0 ? s.dy_max : 0;
  std::vector<int> lo((size_t) s.span,0x7fffffff),hi((size_t) s.span,-0x7fffffff),cnt((size_t) s.span,0);
  for (size_t i=0; i < ncells; i++)
    {
      const size_t k=(size_t) (cells[i].dy-s.dy_min);
      lo[k]=std::min(lo[k],cells[i].dx);
      hi[k]=std::max(hi[k],cells[i].dx);
      cnt[k]++;
    }
  const int centre2=lo[0]+hi[0];                             // (row dy_min has a cell)
  s.half.assign((size_t) s.span,-1);
  for (size_t k=0; k < (size_t) s.span; k++)
    {
      if (cnt[k] == 0)
        {
          s.full=false;
          continue;
        }
      if (cnt[k] != hi[k]-lo[k]+1)
        return false;                                        // a gap in the row
      if ((lo[k]+hi[k] != centre2) || ((centre2 & 1) != 0))
        return false;                                        // runs are not about one centre column
      s.half[k]=(hi[k]-lo[k])/2;
      s.hmax=std::max(s.hmax,s.half[k]);
      s.widths.push_back(s.half[k]);
    }
  s.cx=centre2/2;
  std::sort(s.widths.begin(),s.widths.end());
  s.widths.erase(std::unique(s.widths.begin(),s.widths.end()),s.widths.end());
  return true;
}

// morph_convex_kernel: kernel rows grouped by level.  Level l (half-width widths[l]) owns
// level_dy[level_first[l] .. level_first[l+1])
static inline void convex_levels(const FlatShape &s,std::vector<int> &level_first,std::vector<int> &level_dy)
{
  for (int h : s.widths)
    {
      level_first.push_back((int) level_dy.size());
      for (int k=0; k < s.span; k++)
        if (s.half[(size_t) k] == h)
          level_dy.push_back(k+s.dy_min);
    }
  level_first.push_back((int) level_dy.size());
}

// morph_rects_kernel: 12 waves x 4 rows = kRectsRows output rows a workgroup; a lane holds one (16-byte pixels)
// or two columns, a wave 64 or 128; the tile it stages
constexpr int kRectsRows=48;
static inline int rects_wave_columns(size_t pixel_bytes) { return pixel_bytes >= 16 ? 64 : 128; }
static inline size_t rects_lds_bytes(const FlatShape &s,size_t pixel_bytes)
{
  return (size_t) (kRectsRows+2*(s.span/2))*(size_t) rects_wave_columns(pixel_bytes)*pixel_bytes;
}

// Whether the union-of-rectangles kernel takes the shape on pixels of `pixel_bytes` (4, 8 or 16): every row
// non-empty, the rows symmetric about the middle row and not widening away from it, at least 16 columns of a
// wave left after the 2*hmax it gives up, the staged tile within the CU's 160 KB, at most 64 levels.
static inline bool rects_takes(const FlatShape &s,size_t pixel_bytes)
{
  if (!s.full || ((s.span & 1) == 0))
    return false;
  const int vmax=s.span/2;
  for (int d=0; d <= vmax; d++)
    {
      if (s.half[(size_t) (vmax+d)] != s.half[(size_t) (vmax-d)])
        return false;
      if ((d > 0) && (s.half[(size_t) (vmax+d)] > s.half[(size_t) (vmax+d-1)]))
        return false;
    }
  return (rects_wave_columns(pixel_bytes)-2*s.hmax >= 16) && (rects_lds_bytes(s,pixel_bytes) <= 160u*1024u) &&
    (s.widths.size() <= 64);
}

// ... and its levels, for a shape rects_takes() accepts: widen[l] = h_l - h_{l-1} (h_{-1} = 0), reach[l] = the
// outermost row at least h_l wide.  Returns their number.
static inline int rects_levels(const FlatShape &s,unsigned char *widen,unsigned char *reach)
{
  const int vmax=s.span/2;
  for (size_t l=0; l < s.widths.size(); l++)
    {
      int outermost=0;
      for (int d=0; d <= vmax; d++)
        if (s.half[(size_t) (vmax+d)] >= s.widths[l])
          outermost=d;
      widen[l]=(unsigned char) (s.widths[l]-(l == 0 ? 0 : s.widths[l-1]));
      reach[l]=(unsigned char) outermost;
    }
  return (int) s.widths.size();
}

} // namespace mh
