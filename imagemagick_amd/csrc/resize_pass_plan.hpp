// What the two-pass kernels of resize.hip read besides the contribution lists, and the launch
// geometry of the horizontal pass.  Host only: tests/cpu/resize_pass_plan_test.cpp checks the tables
// against the lists they were made from.  `Table` is a TapTable (resize_filter.hpp): out_size,
// max_taps, start[], count[], weight[tap][out].
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace mh {

constexpr double kPassQuantumScale=1.0/65535.0;      // kQuantumScale (mh_internal.hpp)

// ------------------------------------------------------------- vertical pass
constexpr int kVerticalRows=4;      // output rows per tile of resize_vertical_kernel
// (A reduction's windows are long and overlap — 4x Lanczos: 25 source rows per output, consecutive outputs four
// rows apart — so a tile of 4 outputs reads 40 rows for 16 new ones, the frame 2.5 times: the pass is bound by
// that traffic, 0.27 ms for 8192^2 -> 8192x2048 Q16.  Sixteen outputs a tile read it 1.4 times but, in the dense
// form, run 88 x 16 multiply-adds for 16 x 25 useful ones: 0.82 ms; profiles/r6_notes/resize_reduction.txt.)

// Per tile of kVerticalRows output rows: the union window of their source rows and the dense
// weights W[tile][k][r] over it (VerticalDenseArgs, resize.hip).
struct VerticalPassPlan
{
  int tiles=0,kmax=1;               // kmax: rows of the widest union window
  std::vector<int> lo,rows;         // [tiles] first source row of the window, its height
  std::vector<unsigned> mask;       // [tiles][kmax] bit r: source row k contributes to output r
  std::vector<double> w,wq;         // [tiles][kmax][kVerticalRows] weight, weight*QuantumScale
};

template<class Table>
static void build_vertical_pass_plan(VerticalPassPlan &p,const Table &table)
{
  constexpr int RY=kVerticalRows;
  p.tiles=(table.out_size+RY-1)/RY;
  p.lo.assign((size_t) p.tiles,0);
  p.rows.assign((size_t) p.tiles,0);
  p.kmax=1;
  for (int t=0; t < p.tiles; t++)
    {
      int lo=0x7fffffff,hi=0;
      for (int y=t*RY; (y < (t+1)*RY) && (y < table.out_size); y++)
        if (table.count[y] > 0)
          {
            lo=std::min(lo,table.start[y]);
            hi=std::max(hi,table.start[y]+table.count[y]);
          }
      if (hi <= lo)
        lo=hi=0;
      p.lo[t]=lo;
      p.rows[t]=hi-lo;
      p.kmax=std::max(p.kmax,hi-lo);
    }
  p.w.assign((size_t) p.tiles*p.kmax*RY,0.0);
  p.wq.assign(p.w.size(),0.0);
  p.mask.assign((size_t) p.tiles*p.kmax,0u);
  for (int y=0; y < table.out_size; y++)
    for (int j=0; j < table.count[y]; j++)
      {
        const int t=y/RY,r=y%RY;
        const size_t row=(size_t) t*p.kmax+(size_t) (table.start[y]+j-p.lo[t]);
        const double wv=table.weight[(size_t) j*table.out_size+(size_t) y];
        p.w[row*RY+r]=wv;
        p.wq[row*RY+r]=wv*kPassQuantumScale;         // contribution.weight*QuantumScale
        p.mask[row]|=1u << r;
      }
}

// ----------------------------------------------------------- horizontal pass
constexpr int kHorizontalTile=256;  // output columns per workgroup

// Per tile of kHorizontalTile output columns: the source span the workgroup stages in LDS.
struct HorizontalSpans
{
  int max_span=1;                   // the widest tile
  int overhang=0;                   // columns a converted tile reads past its span: every lane runs maxt taps
  int maxt=8;                       // tap count of the converted-tile kernel: 4, 6, 7 or 8
};
struct HorizontalPassPlan : HorizontalSpans
{
  std::vector<int> tile_lo;         // [tiles] first source column
  std::vector<int> tile_span;       // [tiles] source columns, then [tiles] the tile's largest tap count
  std::vector<double> wq;           // [tap][out] weight*QuantumScale
};

template<class Table>
static void build_horizontal_pass_plan(HorizontalPassPlan &p,const Table &table)
{
  p.wq.resize(table.weight.size());
  for (size_t i=0; i < p.wq.size(); i++)
    p.wq[i]=table.weight[i]*kPassQuantumScale;       // contribution.weight*QuantumScale
  const int tiles=(table.out_size+kHorizontalTile-1)/kHorizontalTile;
  p.tile_lo.assign((size_t) tiles,0);
  p.tile_span.assign((size_t) 2*tiles,0);
  // (a 4x Lanczos enlargement has 6 or 7 contributions per output: 7 taps, not 8)
  p.maxt=table.max_taps <= 4 ? 4 : (table.max_taps <= 6 ? 6 : (table.max_taps <= 7 ? 7 : 8));
  p.max_span=1;                     // the widest tile decides how many rows fit in LDS
  p.overhang=0;
  for (int t=0; t < tiles; t++)
    {
      const int x0=t*kHorizontalTile,x1=std::min(x0+kHorizontalTile,table.out_size);
      int lo=table.start[x0],hi=0,taps=0,reach=0;
      for (int x=x0; x < x1; x++)
        {
          lo=std::min(lo,table.start[x]);
          hi=std::max(hi,table.start[x]+table.count[x]);
          taps=std::max(taps,table.count[x]);
          reach=std::max(reach,table.start[x]+p.maxt);      // the converted-tile kernel reads MAXT samples per output
        }
      hi=std::max(hi,lo);
      p.tile_lo[t]=lo;
      p.tile_span[t]=hi-lo;
      p.tile_span[tiles+t]=taps;    // (run by every lane of the converted-tile kernel)
      p.max_span=std::max(p.max_span,hi-lo);
      p.overhang=std::max(p.overhang,reach-hi);
    }
}

// Which of the seven horizontal kernels runs, and its tile: up to eight taps a tile of samples
// converted to double (resize_horizontal_cvt_kernel<4|6|7|8>) while a row of it stays within 150 KB;
// otherwise the plain tile of Quantum samples (resize_horizontal_kernel<8|16|32|0>, 0 = any number
// of taps).  Rows a tile: what 60 KB hold, 1 .. 16.
struct HorizontalLaunch
{
  bool fits=false;                  // false: a single row of the plain tile is over 150 KB
  bool converted=false;
  int maxt=0;                       // the kernel's MAXT
  int lds_span=0;                   // columns of a tile row
  int tile_rows=0;
  size_t lds=0;                     // bytes
};

static inline HorizontalLaunch horizontal_launch(const HorizontalSpans &p,int max_taps,int channels,
  size_t quantum_bytes)
{
  constexpr size_t budget=60u*1024u,limit=150u*1024u;
  HorizontalLaunch g;
  g.converted=(max_taps <= 8) && ((size_t) (p.max_span+p.overhang)*(size_t) channels*sizeof(double) <= limit);
  g.lds_span=g.converted ? p.max_span+p.overhang : p.max_span;
  g.maxt=g.converted ? p.maxt : (max_taps <= 8 ? 8 : (max_taps <= 16 ? 16 : (max_taps <= 32 ? 32 : 0)));
  const size_t row=(size_t) g.lds_span*(size_t) channels*(g.converted ? sizeof(double) : quantum_bytes);
  g.fits=row <= limit;
  if (!g.fits)
    return g;
  g.tile_rows=(int) std::min<size_t>(std::max<size_t>(budget/row,1),16);
  g.lds=row*(size_t) g.tile_rows;
  return g;
}

} // namespace mh
