// Erode and Dilate (MorphologyPrimitive, MagickCore/morphology.c:2980-3036) with a flat kernel whose active cells
// are one centred run per kernel row: morph_convex_kernel for any such kernel, morph_rects_kernel for those that are
// a union of centred rectangles, and the host routing between them, the gray-row-band and padded-RGB forms of the
// latter and the generic kernel of morphology.hip.  The shape analysis and the tables are morph_flat_plan.hpp's.
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "morph_flat_plan.hpp"

#include <cmath>

namespace mh {

// ------------------------------------------------ Erode / Dilate, convex flat kernels
// Disk, Diamond, Octagon, Square, Rectangle, Plus ...: every kernel row's active
// cells are ONE run [cx-h, cx+h] about a common centre column.  min/max are exact,
// so any evaluation order gives the reference's bits; instead of visiting every
// active cell (Disk:15 = 709) the kernel uses
//     result(x,y) = max_k  M_{h_k}(x+cx, y+dy_k),   M_h(x,y) = max_{|d|<=h} in(x+d, y)
// and builds the row-window maxima M_h incrementally over the kernel's DISTINCT
// half-widths h_0 < h_1 < ... (Disk:15: 10 levels):
//   raw tile (edge-clamped, coalesced loads) -> LDS
//   for each level l:  phase 1  plane(y,x) = max(plane(y,x), raw(y, x+cx+-d), h_{l-1} < d <= h_l)
//                      phase 2  every kernel row k of level l: out[r] = max(out[r], plane(y_r+dy_k, x))
// A 64 x 32 output tile costs ~2*hmax+1 raw reads per tile pixel plus one plane
// read per (kernel row, output) instead of one read per (active cell, output).
struct ConvexArgs
{
  const void *src;
  void *dst;
  int columns,rows;
  int cx;                     // centre column offset of the runs (dx of the run centres)
  int hmax;                   // widest half-width
  int top,bottom;             // kernel rows above / below the output row
  int nlevels;
  const int *level_h;         // [nlevels] ascending distinct half-widths
  const int *level_first;     // [nlevels+1] index into level_dy
  const int *level_dy;        // dy of every kernel row, grouped by level
  uint32_t copy_mask;
  unsigned long long *changed;
};

constexpr int kCTW=64;        // tile columns (= lanes)
constexpr int kCTR=32;        // tile rows; each of the kCWaves waves owns kCTR/kCWaves output rows
// waves per LDS tile: 8 (4 per SIMD with two tiles per CU) for small kernels, 16 for large ones
// (measured on 16384^2: Disk:15 7.6 / 6.1 / 5.5 ms with 4 / 8 / 16 waves, Disk:5 2.2 vs 2.8 ms with 8 vs 16)

template<typename Q,int C> struct PixelMinMax
{
  static __device__ __forceinline__ void apply(Q (&a)[C],const Q (&b)[C],bool take_max)
  {
    if constexpr ((sizeof(Q) == 2) && ((C & 1) == 0))
      {
        typedef unsigned short U2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int p=0; p < C/2; p++)
          {
            U2 va={(unsigned short) a[2*p],(unsigned short) a[2*p+1]};
            U2 vb={(unsigned short) b[2*p],(unsigned short) b[2*p+1]};
            U2 r=take_max ? __builtin_elementwise_max(va,vb) : __builtin_elementwise_min(va,vb);
            a[2*p]=(Q) r[0];
            a[2*p+1]=(Q) r[1];
          }
      }
    else
      {
#pragma unroll
        for (int c=0; c < C; c++)
          {
            if (take_max)
              { if (b[c] > a[c]) a[c]=b[c]; }          // morphology.c:3025-3026
            else
              { if (b[c] < a[c]) a[c]=b[c]; }          // morphology.c:2997-2998
          }
      }
  }
};

template<typename Q,int C,bool DILATE,int kCWaves>
__global__ __launch_bounds__(64*kCWaves)
void morph_convex_kernel(ConvexArgs args)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int W=args.columns,H=args.rows;
  const int hmax=args.hmax,top=args.top;
  const int tile_rows=kCTR+top+args.bottom;
  const int raw_w=kCTW+2*hmax;
  Q *raw=reinterpret_cast<Q *>(smem_raw);
  Q *plane=raw+(size_t) tile_rows*raw_w*C;
  const Q *src=static_cast<const Q *>(args.src);
  Q *dst=static_cast<Q *>(args.dst);
  const size_t pitch=(size_t) W*C;
  const int bx=(int) blockIdx.x*kCTW,by=(int) blockIdx.y*kCTR;
  const int lane=(int) (threadIdx.x & 63);
  const int wave=__builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));

  // raw tile: tile column t is image column bx + cx - hmax + t (edge clamp, cache.c:2663-2679)
  {
    constexpr int BATCH=6;
    const int items=tile_rows*raw_w;
    for (int i0=(int) threadIdx.x; i0 < items; i0+=64*kCWaves*BATCH)
      {
        Q v[BATCH][C];
#pragma unroll
        for (int k=0; k < BATCH; k++)
          {
            int idx=i0+64*kCWaves*k;
            idx=idx < items ? idx : items-1;
            const int ty=idx/raw_w,tx=idx-ty*raw_w;
            int sx=bx+args.cx-hmax+tx,sy=by-top+ty;
            sx=sx < 0 ? 0 : (sx > W-1 ? W-1 : sx);
            sy=sy < 0 ? 0 : (sy > H-1 ? H-1 : sy);
            load_pixel<Q,C>(src+(size_t) sy*pitch+(size_t) sx*C,v[k]);
          }
#pragma unroll
        for (int k=0; k < BATCH; k++)
          if (i0+64*kCWaves*k < items)
            store_pixel<Q,C>(raw+(size_t) (i0+64*kCWaves*k)*C,v[k]);
      }
  }
  // accumulators: Erode starts from the output pixel itself, Dilate from 0 (morphology.c:2905-2912)
  constexpr int R=kCTR/kCWaves;
  const int x=bx+lane;
  const int xc=x < W ? x : W-1;
  Q out[R][C],center[R][C];
#pragma unroll
  for (int r=0; r < R; r++)
    {
      int y=by+wave*R+r;
      y=y < H ? y : H-1;
      load_pixel<Q,C>(src+(size_t) y*pitch+(size_t) xc*C,center[r]);
#pragma unroll
      for (int c=0; c < C; c++)
        out[r][c]=DILATE ? (Q) 0 : center[r][c];
    }
  __syncthreads();

  int h_prev=-1;
  for (int l=0; l < args.nlevels; l++)
    {
      const int h=args.level_h[l];
      // phase 1: widen the row-window maxima of every tile row to half-width h.  Four
      // rows per step: their LDS reads are independent, so one latency covers all four.
      constexpr int RB=4;
      for (int t0=wave; t0 < tile_rows; t0+=kCWaves*RB)
        {
          Q m[RB][C];
          const Q *line[RB];
#pragma unroll
          for (int k=0; k < RB; k++)
            {
              int ty=t0+kCWaves*k;
              ty=ty < tile_rows ? ty : tile_rows-1;
              line[k]=raw+((size_t) ty*raw_w+(size_t) (lane+hmax))*C;
              if (h_prev < 0)
                load_pixel<Q,C>(line[k],m[k]);
              else
                load_pixel<Q,C>(plane+((size_t) ty*kCTW+lane)*C,m[k]);
            }
          for (int d=(h_prev < 0 ? 1 : h_prev+1); d <= h; d++)
            {
              Q a[RB][C],b[RB][C];
#pragma unroll
              for (int k=0; k < RB; k++)
                {
                  load_pixel<Q,C>(line[k]-(size_t) d*C,a[k]);
                  load_pixel<Q,C>(line[k]+(size_t) d*C,b[k]);
                }
#pragma unroll
              for (int k=0; k < RB; k++)
                {
                  PixelMinMax<Q,C>::apply(m[k],a[k],DILATE);
                  PixelMinMax<Q,C>::apply(m[k],b[k],DILATE);
                }
            }
#pragma unroll
          for (int k=0; k < RB; k++)
            {
              int ty=t0+kCWaves*k;
              if (ty < tile_rows)
                store_pixel<Q,C>(plane+((size_t) ty*kCTW+lane)*C,m[k]);
            }
        }
      __syncthreads();
      // phase 2: the kernel rows whose run has this half-width
      for (int i=args.level_first[l]; i < args.level_first[l+1]; i++)
        {
          const int dy=args.level_dy[i];
          const Q *col=plane+((size_t) (wave*R+top+dy)*kCTW+lane)*C;
#pragma unroll
          for (int r=0; r < R; r++)
            {
              Q v[C];
              load_pixel<Q,C>(col+(size_t) r*kCTW*C,v);
              PixelMinMax<Q,C>::apply(out[r],v,DILATE);
            }
        }
      __syncthreads();
      h_prev=h;
    }
  unsigned changed=0;
#pragma unroll
  for (int r=0; r < R; r++)
    {
      const int y=by+wave*R+r;
      if ((x < W) && (y < H))
        {
          Q res[C];
#pragma unroll
          for (int c=0; c < C; c++)
            {
              if ((args.copy_mask >> c) & 1u)
                {
                  res[c]=center[r][c];
                  continue;
                }
              double pixel=(double) out[r][c];
              if (fabs(pixel-(double) center[r][c]) >= kEps)
                changed++;
              res[c]=QuantumOps<Q>::clamp(pixel);
            }
          store_pixel<Q,C>(dst+(size_t) y*pitch+(size_t) x*C,res);
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}

template<typename Q,int C>
static MhStatus launch_convex(bool dilate,const ConvexArgs &args,dim3 grid,size_t lds,hipStream_t stream)
{
  const auto launch=[&](auto kernel,int waves) { return launch_dynamic_lds(kernel,grid,dim3(64*waves),lds,stream,args); };
  const bool large=(args.top+args.bottom) >= 16;
  if (dilate)
    return large ? launch(&morph_convex_kernel<Q,C,true,16>,16) : launch(&morph_convex_kernel<Q,C,true,8>,8);
  return large ? launch(&morph_convex_kernel<Q,C,false,16>,16) : launch(&morph_convex_kernel<Q,C,false,8>,8);
}

// ------------------------------------------------ Erode / Dilate, symmetric convex kernels
// A flat kernel whose rows are centred runs, symmetric about a centre row, with half-widths that do
// not grow away from it (Disk, Square, Rectangle, Diamond, Octagon, Plus ...) is the union of the
// centred rectangles  Rect(h_l, v_l),  h_0 < h_1 < ... < h_L  the distinct half-widths and v_l the
// largest |dy| whose row is at least h_l wide (v_0 > v_1 > ... > v_L).  With Row(h) = Row(h_0) +
// Row(h_1-h_0) + ... (Minkowski sums) and because dilation distributes over unions,
//     out = Row(h_0)[ Col(v_0) in  v  Row(h_1-h_0)[ Col(v_1) in  v  ... Row(h_L-h_{L-1})[ Col(v_L) in ] ] ]
// evaluated from the inside out:   C <- Col(v_l) in  (widened from Col(v_{l+1}) in: v_l grows),
//                                  S <- Row(h_l-h_{l-1})[ C v S ].
// 2 v_0 + 2 h_L + L+1 compares per pixel (Disk:15: 71 against the 709 cells), all min/max, so
// the result has the reference's bits (morphology.c:2980-3036) whatever the order.
//
// MI355X mapping: lane = two adjacent columns, a wave = 128 columns x SY rows held in VGPRs (C
// and S).  Col() reads the lane's own columns of the staged tile (ds_read_b128, conflict free,
// wave-uniform row offsets); Row(d) is d applications of Row(1), whose two neighbour columns
// that live in the next lane come over with one v_mov_b32_dpp wave_shr:1 / wave_shl:1 each — no
// LDS traffic and no barrier between the levels.  The columns within hmax of the wave's edges
// fill with garbage (one per Row(1)) and are not stored: a workgroup produces 128-2*hmax columns.
struct RectsArgs
{
  const void *src;            // Q16 or float Quantum, 4-byte multiples per pixel
  void *dst;
  int columns,rows;
  int cx,cy;                  // centre of the shape relative to the output pixel
  int hmax,vmax;              // half-width of the widest row, half-height
  int nlevels;
  int tiles_x,tiles_y,tiles_per_xcd;
  uint32_t copy_mask;
  unsigned long long *changed;
  unsigned char widen[64];    // [nlevels]  h_l - h_{l-1}  (h_{-1} = 0)
  unsigned char reach[64];    // [nlevels]  v_l
};

template<bool DILATE>
static __device__ __forceinline__ uint32_t pk_pick(uint32_t a,uint32_t b)
{
  typedef unsigned short U2 __attribute__((ext_vector_type(2)));
  const U2 va=__builtin_bit_cast(U2,a),vb=__builtin_bit_cast(U2,b);
  return __builtin_bit_cast(uint32_t,DILATE ? __builtin_elementwise_max(va,vb) : __builtin_elementwise_min(va,vb));
}

// one 32-bit word of samples: two Q16 channels (packed compare) or one float channel.  The float
// forms are v_max_f32 / v_min_f32: a NaN operand yields the other one, which is what the
// reference's `if (pixels[i] > pixel)` does with a NaN neighbour (morphology.c:2995-3030).
// (fmaxf / fminf: hipcc canonicalises both operands first — a v_max_f32 x,x each — and fuses pairs
// into v_max3_f32 / v_min3_f32.  The bare instructions through inline asm measured slower, 5.3
// against 4.8 ms for Dilate Disk:15 on 16384^2 float RGBA: the scheduler cannot see into them.)
template<typename Q,bool DILATE>
static __device__ __forceinline__ uint32_t word_pick(uint32_t a,uint32_t b)
{
  if constexpr (sizeof(Q) == 2)
    return pk_pick<DILATE>(a,b);
  else
    {
      const float fa=__builtin_bit_cast(float,a),fb=__builtin_bit_cast(float,b);
      return __builtin_bit_cast(uint32_t,DILATE ? __builtin_fmaxf(fa,fb) : __builtin_fminf(fa,fb));
    }
}

template<typename Q,bool DILATE>
static __device__ __forceinline__ uint32_t word_pick3(uint32_t a,uint32_t b,uint32_t c)
{
  return word_pick<Q,DILATE>(word_pick<Q,DILATE>(a,b),c);
}

// Q: uint16_t (2 or 4 channels) or float (1, 2 or 4 channels: the reference's default build is
// HDRI; min/max are exact in any type).  A lane holds SX columns = WPR words; RGBA float is one
// column per lane (a wave keeps 64-2*hmax of its 64 columns).
template<typename Q,int C,bool DILATE,int SY,int NWAVES>
__global__ __launch_bounds__(64*NWAVES)
void morph_rects_kernel(RectsArgs args)
{
  constexpr int PXB=C*(int) sizeof(Q);         // bytes per pixel
  static_assert((PXB % 4) == 0,"whole 32-bit words per pixel");
  constexpr int NW=PXB/4;                      // 32-bit words per pixel
  constexpr int SX=NW >= 4 ? 1 : 2;            // columns per lane
  constexpr int WPR=SX*NW;                     // words a lane holds per row
  constexpr bool kFloat=sizeof(Q) == 4;
  constexpr int TH=SY*NWAVES;                  // output rows per workgroup
  typedef uint32_t Group __attribute__((ext_vector_type(WPR)));
  typedef Group __attribute__((aligned(4))) LooseGroup;      // global memory: pixel alignment only
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Group *tile=reinterpret_cast<Group *>(smem_raw);           // [TH+2*vmax][64]
  const int W=args.columns,H=args.rows;
  const int hmax=args.hmax,vmax=args.vmax;
  const int tid=(int) threadIdx.x,lane=tid & 63;
  const int wave=__builtin_amdgcn_readfirstlane(tid >> 6);
  // consecutive workgroup ids go to different XCDs: give each XCD a contiguous run of tiles,
  // row-major, so that the halo a tile shares with its neighbours is in that XCD's L2
  const int id=((int) blockIdx.x & 7)*args.tiles_per_xcd+((int) blockIdx.x >> 3);
  if (id >= args.tiles_x*args.tiles_y)
    return;
  const int tile_y=id/args.tiles_x,tile_x=id-tile_y*args.tiles_x;
  const int valid_w=64*SX-2*hmax;
  const int bx=tile_x*valid_w,by=tile_y*TH;
  const int tile_rows=TH+2*vmax;

  // ---- stage the edge-clamped source window (cache.c:2663-2679): tile column t is image
  // column bx+cx-hmax+t, tile row q is image row by+cy-vmax+q
  {
    // a thread keeps its columns and walks down the rows NWAVES apart: the column clamp and the
    // in-frame test are done once, a row costs its clamp and one (wave-uniform, 64-bit) offset
    const int sx=bx+args.cx-hmax+SX*lane,sy0=by+args.cy-vmax;
    const bool inside=(sx >= 0) && (sx+SX-1 <= W-1);
    unsigned xoff[SX];
#pragma unroll
    for (int j=0; j < SX; j++)
      {
        int x=sx+j;
        x=x < 0 ? 0 : (x > W-1 ? W-1 : x);
        xoff[j]=(unsigned) x*(unsigned) PXB;
      }
    const unsigned row_bytes=(unsigned) W*(unsigned) PXB;
    const unsigned char *base=reinterpret_cast<const unsigned char *>(args.src);
    constexpr int BATCH=4;                       // Disk:15: 7 rows per thread (12 waves), two round trips
    for (int q0=wave; q0 < tile_rows; q0+=NWAVES*BATCH)
      {
        Group g[BATCH];
#pragma unroll
        for (int k=0; k < BATCH; k++)
          {
            int q=q0+NWAVES*k;
            q=q < tile_rows ? q : tile_rows-1;
            int sy=sy0+q;
            sy=sy < 0 ? 0 : (sy > H-1 ? H-1 : sy);
            const unsigned char *row=base+(size_t) sy*row_bytes;
            if (inside)
              g[k]=*reinterpret_cast<const LooseGroup *>(row+xoff[0]);
            else
              {
#pragma unroll
                for (int j=0; j < SX; j++)
#pragma unroll
                  for (int w=0; w < NW; w++)
                    g[k][j*NW+w]=*reinterpret_cast<const uint32_t *>(row+xoff[j]+4*w);
              }
          }
#pragma unroll
        for (int k=0; k < BATCH; k++)
          if (q0+NWAVES*k < tile_rows)
            tile[(q0+NWAVES*k)*64+lane]=g[k];
      }
  }
  __syncthreads();

  // ---- the wave's SY output rows: tile rows wave*SY+vmax+i
  const Group *centre=tile+(size_t) (wave*SY+vmax)*64+lane;
  uint32_t column[SY][WPR],spread[SY][WPR];    // C and S of the header
  // The rows a fold depth takes in slide: at depth k output row i needs tile rows i-k and i+k, and
  // row i-k = row (i+1)-(k+1) was read one depth earlier for output row i+1.  `upper` holds the
  // rows 0-j (j = k-SY+1 .. k) in slot j mod SY, `lower` the rows SY-1+j: a depth costs two row
  // reads instead of 2*SY (the LDS pipe, not the vector unit, set the pace of the fold), and
  // with the depths unrolled SY at a time every slot is a compile-time register.
  Group upper[SY],lower[SY];
#pragma unroll
  for (int i=0; i < SY; i++)
    {
      const Group g=centre[i*64];
      upper[(SY-i)%SY]=g;                      // row i = row 0-(-i)
      lower[(i+1)%SY]=g;                       // row i = row SY-1+(i-SY+1)
#pragma unroll
      for (int p=0; p < WPR; p++)
        {
          column[i][p]=g[p];
          spread[i][p]=DILATE ? 0u : (kFloat ? 0x7f800000u : 0xffffffffu);   // 0 / QuantumRange or +inf
        }
    }
  // lane l keeps level l's reach and widening: a v_readlane per level instead of a load from the
  // kernel arguments
  const int lane_reach=lane < args.nlevels ? (int) args.reach[lane] : 0;
  const int lane_widen=lane < args.nlevels ? (int) args.widen[lane] : 0;
  // every level whose reach the fold depth has arrived at: merge the column windows into the
  // spread and widen it (the levels' reaches grow as l falls)
  int level=args.nlevels-1;
  auto settle=[&](int depth)
  {
    while ((level >= 0) && (__builtin_amdgcn_readlane(lane_reach,level) <= depth))
      {
#pragma unroll
        for (int i=0; i < SY; i++)
#pragma unroll
          for (int p=0; p < WPR; p++)
            spread[i][p]=word_pick<Q,DILATE>(spread[i][p],column[i][p]);
        const int widen=__builtin_amdgcn_readlane(lane_widen,level);
        for (int step=0; step < widen; step++)
          {
            // Row(1): every column takes in its two neighbours.  Two columns a b per lane share
            // their pair maximum: a <- b' v (a v b), b <- (a v b) v a' (b', a': the neighbour lanes');
            // one column per lane: a <- a' v a v a''
#pragma unroll
            for (int i=0; i < SY; i++)
#pragma unroll
              for (int w=0; w < NW; w++)
                {
                  // wave_shr:1 — lane n reads lane n-1 (0x138); wave_shl:1 — lane n reads lane n+1 (0x130)
                  if constexpr (SX == 2)
                    {
                      const uint32_t a=spread[i][w],b=spread[i][NW+w];
                      const uint32_t left=(uint32_t) __builtin_amdgcn_mov_dpp((int) b,0x138,0xf,0xf,true);
                      const uint32_t right=(uint32_t) __builtin_amdgcn_mov_dpp((int) a,0x130,0xf,0xf,true);
                      const uint32_t both=word_pick<Q,DILATE>(a,b);
                      spread[i][w]=word_pick<Q,DILATE>(left,both);
                      spread[i][NW+w]=word_pick<Q,DILATE>(both,right);
                    }
                  else
                    {
                      const uint32_t a=spread[i][w];
                      const uint32_t left=(uint32_t) __builtin_amdgcn_mov_dpp((int) a,0x138,0xf,0xf,true);
                      const uint32_t right=(uint32_t) __builtin_amdgcn_mov_dpp((int) a,0x130,0xf,0xf,true);
                      spread[i][w]=word_pick3<Q,DILATE>(left,a,right);
                    }
                }
          }
        level--;
      }
  };
  settle(0);
  for (int k0=1; k0 <= vmax; k0+=SY)
    {
#pragma unroll
      for (int u=0; u < SY; u++)
        {
          const int k=k0+u;                    // k mod SY = (1+u) mod SY
          if (k > vmax)
            break;
          upper[(1+u)%SY]=centre[-k*64];
          lower[(1+u)%SY]=centre[(SY-1+k)*64];
#pragma unroll
          for (int i=0; i < SY; i++)
            {
              // row i-k is row 0-(k-i), row i+k is row SY-1+(k+i-SY+1)
              const Group &above=upper[(1+u+SY-i)%SY];
              const Group &below=lower[(2+u+i)%SY];
#pragma unroll
              for (int p=0; p < WPR; p++)
                column[i][p]=word_pick3<Q,DILATE>(column[i][p],above[p],below[p]);
            }
          settle(k);
        }
    }

  // ---- copy out: morphology.c:3180-3196 (channels without the update trait keep the source
  // value; `changed` counts the updated samples that differ from the source)
  unsigned changed=0;
  const int u0=SX*lane-hmax;                   // first of the lane's columns within the valid span
  const bool centred=(args.cx == 0) && (args.cy == 0);
  if (DILATE && (args.copy_mask == 0u) && (args.changed == nullptr))
    {
      // every channel updated, nobody counts: the maxima are the result
      const bool whole=(u0 >= 0) && (u0+SX-1 < valid_w) && (bx+u0+SX-1 < W);
#pragma unroll
      for (int i=0; i < SY; i++)
        {
          const int y=by+wave*SY+i;
          if (y >= H)
            break;
          unsigned char *out=reinterpret_cast<unsigned char *>(args.dst)+(size_t) y*((size_t) W*(size_t) PXB);
          Group result;
#pragma unroll
          for (int p=0; p < WPR; p++)
            result[p]=spread[i][p];
          if (whole)
            *reinterpret_cast<LooseGroup *>(out+(unsigned) (bx+u0)*(unsigned) PXB)=result;
          else
            {
#pragma unroll
              for (int j=0; j < SX; j++)
                if ((u0+j >= 0) && (u0+j < valid_w) && (bx+u0+j < W))
#pragma unroll
                  for (int w=0; w < NW; w++)
                    *reinterpret_cast<uint32_t *>(out+(unsigned) (bx+u0+j)*(unsigned) PXB+4*w)=result[j*NW+w];
            }
        }
      return;
    }
#pragma unroll
  for (int i=0; i < SY; i++)
    {
      const int y=by+wave*SY+i;
      if (y >= H)
        break;
      unsigned char *out_row=reinterpret_cast<unsigned char *>(args.dst)+(size_t) y*((size_t) W*(size_t) PXB);
      const unsigned char *in_row=reinterpret_cast<const unsigned char *>(args.src)+(size_t) y*((size_t) W*(size_t) PXB);
      bool ok[SX];
#pragma unroll
      for (int j=0; j < SX; j++)
        ok[j]=(u0+j >= 0) && (u0+j < valid_w) && (bx+u0+j < W);
      Group original;
      bool all=true;
#pragma unroll
      for (int j=0; j < SX; j++)
        all=all && ok[j];
      if (centred)
        original=centre[i*64];                 // the output pixel is the centre of its own window
      else if (all)
        original=*reinterpret_cast<const LooseGroup *>(in_row+(unsigned) (bx+u0)*(unsigned) PXB);
      else
        {
#pragma unroll
          for (int j=0; j < SX; j++)
#pragma unroll
            for (int w=0; w < NW; w++)
              original[j*NW+w]=ok[j] ? *reinterpret_cast<const uint32_t *>(in_row+(unsigned) (bx+u0+j)*(unsigned) PXB+4*w) : 0u;
        }
      Group result;
#pragma unroll
      for (int p=0; p < WPR; p++)
        {
          if constexpr (kFloat)
            {
              // one channel per word.  Erode starts from the output pixel itself
              // (morphology.c:2905-2912): a NaN there stays (no `<` is true against it)
              const int c=p % NW;
              const uint32_t mine_bits=original[p];    // (a copy: __builtin_bit_cast of the vector
              const float mine=__builtin_bit_cast(float,mine_bits);   // element itself reads element 0)
              uint32_t value=spread[i][p];
              if (!DILATE)
                value=mine != mine ? mine_bits : word_pick<Q,false>(value,mine_bits);
              const bool keep=((args.copy_mask >> c) & 1u) != 0u;
              result[p]=keep ? mine_bits : value;
              // morphology.c:3195: fabs(pixel-p[center+i]) >= MagickEpsilon
              if (!keep && ok[p/NW] &&
                  (fabs((double) __builtin_bit_cast(float,value)-(double) mine) >= kEps))
                changed++;
            }
          else
            {
              // Erode starts from the output pixel itself (morphology.c:2905-2912)
              const uint32_t value=DILATE ? spread[i][p] : pk_pick<false>(spread[i][p],original[p]);
              const int c0=2*(p % NW);             // channels of this word's halves
              uint32_t keep=0u;
              keep|=((args.copy_mask >> c0) & 1u) != 0u ? 0x0000ffffu : 0u;
              keep|=((args.copy_mask >> (c0+1)) & 1u) != 0u ? 0xffff0000u : 0u;
              result[p]=(original[p] & keep) | (value & ~keep);
              const uint32_t differs=(value ^ original[p]) & ~keep;
              if (ok[p/NW])
                changed+=((differs & 0xffffu) != 0u ? 1u : 0u)+((differs >> 16) != 0u ? 1u : 0u);
            }
        }
      if (all)
        *reinterpret_cast<LooseGroup *>(out_row+(unsigned) (bx+u0)*(unsigned) PXB)=result;
      else
        {
#pragma unroll
          for (int j=0; j < SX; j++)
            if (ok[j])
#pragma unroll
              for (int w=0; w < NW; w++)
                *reinterpret_cast<uint32_t *>(out_row+(unsigned) (bx+u0+j)*(unsigned) PXB+4*w)=result[j*NW+w];
        }
    }
  if (args.changed != nullptr)
    {
      changed=wave_sum(changed);
      if ((lane == 0) && (changed != 0))
        atomicAdd(args.changed,(unsigned long long) changed);
    }
}

// 12 waves x 4 rows: the kRectsRows output rows a workgroup of morph_flat_plan.hpp
template<typename Q,int C>
static MhStatus launch_rects(bool dilate,const RectsArgs &args,size_t lds,hipStream_t stream)
{
  const dim3 grid((unsigned) (8*args.tiles_per_xcd)),block(64*12);
  return dilate ? launch_dynamic_lds(&morph_rects_kernel<Q,C,true,4,12>,grid,block,lds,stream,args) :
    launch_dynamic_lds(&morph_rects_kernel<Q,C,false,4,12>,grid,block,lds,stream,args);
}

static size_t sample_bytes(const View &v) { return v.quantum == MH_QUANTUM_U16 ? sizeof(uint16_t) : sizeof(float); }
static size_t pixel_bytes(const View &v) { return (size_t) v.channels*sample_bytes(v); }

// morph_convex_kernel's raw tile and plane
static size_t convex_lds_bytes(const FlatShape &s,size_t bytes)
{
  return (size_t) (kCTR+s.top+s.bottom)*((size_t) (kCTW+2*s.hmax)+(size_t) kCTW)*bytes;
}

static MhStatus morph_convex(const View &src,const View &dst,bool dilate,const FlatShape &s,const Roles &roles,
  unsigned long long *changed)
{
  // distinct half-widths ascending, kernel rows grouped by level
  std::vector<int> level_first,level_dy;
  convex_levels(s,level_first,level_dy);
  Temp d_h,d_first,d_dy;
  MH_TRY(upload_table(d_h,src.device,src.stream,s.widths.data(),s.widths.size()*sizeof(int)));
  MH_TRY(upload_table(d_first,src.device,src.stream,level_first.data(),level_first.size()*sizeof(int)));
  MH_TRY(upload_table(d_dy,src.device,src.stream,level_dy.data(),level_dy.size()*sizeof(int)));
  ConvexArgs a;
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.columns=(int) src.columns;
  a.rows=(int) src.rows;
  a.cx=s.cx;
  a.hmax=s.hmax;
  a.top=s.top;
  a.bottom=s.bottom;
  a.nlevels=(int) s.widths.size();
  a.level_h=d_h.as<int>();
  a.level_first=d_first.as<int>();
  a.level_dy=d_dy.as<int>();
  a.copy_mask=roles.copy_mask;
  a.changed=changed;
  const size_t lds=convex_lds_bytes(s,pixel_bytes(src));
  dim3 grid((unsigned) ((src.columns+kCTW-1)/kCTW),(unsigned) ((src.rows+kCTR-1)/kCTR));
  ProfileScope prof("morph_convex",src.stream);
  return dispatch_layout(src.quantum,src.channels,[&](auto L) {
    return launch_convex<typename decltype(L)::Q,L.C>(dilate,a,grid,lds,src.stream); });
}

// the union-of-rectangles kernel on a frame of 4-, 8- or 16-byte pixels, for a shape rects_takes() accepts
static MhStatus morph_rects(const View &src,const View &dst,bool dilate,const FlatShape &s,const Roles &roles,
  unsigned long long *changed)
{
  RectsArgs a;
  a.nlevels=rects_levels(s,a.widen,a.reach);
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.columns=(int) src.columns;
  a.rows=(int) src.rows;
  a.cx=s.cx;
  a.vmax=s.span/2;
  a.cy=s.dy_min+a.vmax;
  a.hmax=s.hmax;
  a.copy_mask=roles.copy_mask;
  a.changed=changed;
  const int valid_w=rects_wave_columns(pixel_bytes(src))-2*s.hmax;
  a.tiles_x=((int) src.columns+valid_w-1)/valid_w;
  a.tiles_y=((int) src.rows+kRectsRows-1)/kRectsRows;
  a.tiles_per_xcd=(a.tiles_x*a.tiles_y+7)/8;
  const size_t lds=rects_lds_bytes(s,pixel_bytes(src));
  ProfileScope prof("morph_rects",src.stream);
  if (src.quantum != MH_QUANTUM_U16)
    {
      if (src.channels == 4)
        return launch_rects<float,4>(dilate,a,lds,src.stream);
      if (src.channels == 2)
        return launch_rects<float,2>(dilate,a,lds,src.stream);
      return launch_rects<float,1>(dilate,a,lds,src.stream);
    }
  if (src.channels == 4)
    return launch_rects<uint16_t,4>(dilate,a,lds,src.stream);
  return launch_rects<uint16_t,2>(dilate,a,lds,src.stream);
}

// A one-channel (gray) Q16 frame — the masks Erode and Dilate are mostly run on — has no 4- or 8-byte pixel for
// the union-of-rectangles kernel's lanes and took morph_convex (Disk:15 on 8192^2: 1.35 ms, an RGBA frame 0.51).
// Its rows cut into four bands ARE the four channels of a frame a quarter as tall (gray_bands_pack_kernel,
// pointwise.hip: the kernel's reach in extra rows between bands, the frame's own edge rows repeated above the first
// and below the last as cache.c:2663-2679 does); minima and maxima are taken per channel, so the result is the
// frame's own.  The change count (morphology.c:3199) is taken while unpacking, over the frame's own samples.
static MhStatus morph_rects_gray_bands(const View &src,const View &dst,bool dilate,const FlatShape &s,
  unsigned long long *changed)
{
  GrayBands bands;
  MH_TRY(bands.pack(src,std::max(s.top,s.bottom)));
  MH_TRY(morph_rects(bands.packed,bands.result,dilate,s,GrayBands::plain_roles(),nullptr));
  return bands.unpack(dst,src.pixels,changed);
}

// A three-channel frame (RGB without alpha: what most photographs are) has 6- or 12-byte pixels and took morph_convex
// (Dilate Disk:15 on 8192^2 Q16: 4.05 ms, an RGBA frame 0.53).  With a fourth, empty channel it is an ordinary
// four-channel frame (rgb_pad_kernel, pointwise.hip); the change count is taken while dropping that channel again.
static MhStatus morph_rects_rgb_padded(const View &src,const View &dst,bool dilate,const FlatShape &s,
  const Roles &roles,unsigned long long *changed)
{
  View padded=src,result=src;
  padded.channels=result.channels=4;
  Temp padded_memory,result_memory;
  MH_TRY(padded_memory.alloc(src.device,padded.bytes(),src.stream));
  MH_TRY(result_memory.alloc(src.device,result.bytes(),src.stream));
  padded.pixels=padded_memory.ptr;
  result.pixels=result_memory.ptr;
  MH_TRY(launch_rgb_pad(src,padded));
  Roles four=roles;
  four.blend=false;
  four.alpha=-1;
  four.copy_mask=roles.copy_mask & 0x7u;
  four.update_mask=0xfu & ~four.copy_mask;
  MH_TRY(morph_rects(padded,result,dilate,s,four,nullptr));
  return launch_rgb_unpad(result,dst,src.pixels,changed);
}

// ------------------------------------------------ the route of a flat kernel
// Decided here, once, from the kernel's shape and the frame's layout, size and channel roles, before anything is
// packed, padded, uploaded or launched: every condition of morph_rects_kernel depends on the shape and on the pixel
// size it would run on (rects_takes), and that size is known for the packed and the padded frame as well.
MhStatus launch_morph_flat(const View &src,const View &dst,bool dilate,const Cell *cells,size_t ncells,
  const Roles &roles,unsigned long long *changed,bool *handled)
{
  FlatShape s;
  *handled=(ncells >= 9) &&                   // tiny kernels: the cell walk is already cheap
    flat_shape(cells,ncells,s) && (s.dy_min <= 0) && (s.dy_max >= 0) && (s.hmax <= 48) && (s.span <= 97) &&
    (src.channels >= 1) && (src.channels <= 4);
  if (!*handled)
    return MH_OK;                              // the generic kernel (morphology.hip)
  const bool is_float=src.quantum != MH_QUANTUM_U16;
  const size_t four=4*sample_bytes(src);      // bytes of a four-channel pixel
  // symmetric shapes: the union-of-rectangles kernel
  if ((option("MAGICKHIP_NO_RECTS") == nullptr) && (!is_float || (option("MAGICKHIP_NO_FLOAT_RECTS") == nullptr)) &&
      (src.columns < (1u << 30)) && (src.rows < (1u << 30)))
    {
      if (!is_float && (src.channels == 1))
        {
          // a gray Q16 frame has no 4-byte pixel: its four row bands, or morph_convex
          const int halo=std::max(s.top,s.bottom);
          if ((option("MAGICKHIP_NO_GRAY_BANDS") == nullptr) && (roles.copy_mask == 0) && (halo >= 1) &&
              GrayBands::fits(src,halo,1l << 18) && rects_takes(s,four))
            return morph_rects_gray_bands(src,dst,dilate,s,changed);
        }
      else if (src.channels == 3)
        {
          // Q16: faster than morph_convex at every size and kernel measured (8192^2 Disk:15 4.02 -> 0.85 ms, Square:1 0.67
          // -> 0.60; 256^2 0.051 -> 0.039).  Float: padding moves 28 bytes a pixel twice (0.70 ms per 8192^2) and
          // morph_convex is quick on its small kernels (Disk:5 0.88 ms, padded 1.24) — only where its tile no longer fits
          // (80 KB, below; from Disk:8 on) and the frame would take the generic kernel (Disk:15: 15.2 ms, padded 1.97)
          const int v=s.span/2,h=s.half[(size_t) v];
          if ((option("MAGICKHIP_NO_RGB_PAD") == nullptr) &&
              (!is_float || option("MAGICKHIP_RGB_PAD_FLOAT_ALWAYS") != nullptr ||
               ((size_t) (kCTR+2*v)*(size_t) (2*kCTW+2*h)*12u > 80u*1024u)) &&
              (src.columns*src.rows >= (size_t) option_long("MAGICKHIP_RGB_PAD_MIN_PIXELS",1l << 16)) &&
              rects_takes(s,four))
            return morph_rects_rgb_padded(src,dst,dilate,s,roles,changed);
        }
      else if (rects_takes(s,pixel_bytes(src)))             // float C = 1, 2, 4 and Q16 C = 2, 4
        return morph_rects(src,dst,dilate,s,roles,changed);
    }
  if (convex_lds_bytes(s,pixel_bytes(src)) <= 80u*1024u)      // keep two workgroups per CU
    return morph_convex(src,dst,dilate,s,roles,changed);
  *handled=false;
  return MH_OK;
}

} // namespace mh
