// MotionBlurImage, RotationalBlurImage, LocalContrastImage, DespeckleImage and WaveletDenoiseImage: the reference's
// loops restated one thread per column (column_grid, layout_dispatch.hpp), fp64 or float as the reference computes,
// in its order.
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include <vector>

#include <cmath>

namespace mh {

// ---------------------------------------------------------------- MotionBlurImage
// effect.c:2347-2560: a 1-D kernel applied along a line of integer offsets, virtual pixels
// edge-clamped, alpha-weighted on Blend channels; fp64 in the reference's order
// (pixel += (k*alpha)*r; gamma += k*alpha).
struct MotionArgs
{
  const void *src;
  void *dst;
  int columns,rows;
  int width;
  const double *kernel;        // [width]
  const int *offset;           // [width][2] = x,y
  uint32_t copy_mask;
  int alpha;                   // alpha channel or -1
};

template<typename Q,int C,bool BLEND>
__global__ __launch_bounds__(256)
void motion_blur_kernel(MotionArgs a)
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x),y=(int) blockIdx.y;
  if (x >= a.columns)
    return;
  const Q *src=static_cast<const Q *>(a.src);
  double pixel[C],gamma=0.0;
#pragma unroll
  for (int c=0; c < C; c++)
    pixel[c]=0.0;
  for (int j=0; j < a.width; j++)
    {
      int sx=x+a.offset[2*j],sy=y+a.offset[2*j+1];
      sx=sx < 0 ? 0 : (sx > a.columns-1 ? a.columns-1 : sx);      // cache.c:2663-2679
      sy=sy < 0 ? 0 : (sy > a.rows-1 ? a.rows-1 : sy);
      Q r[C];
      load_pixel<Q,C>(src+((size_t) sy*a.columns+sx)*C,r);
      const double k=a.kernel[j];
      if (BLEND)
        {
          const double alpha=kQS*(double) r[C-1];
          const double weight=k*alpha;
#pragma unroll
          for (int c=0; c < C-1; c++)
            pixel[c]+=weight*(double) r[c];
          gamma+=weight;
          pixel[C-1]+=k*(double) r[C-1];
        }
      else
        {
#pragma unroll
          for (int c=0; c < C; c++)
            pixel[c]+=k*(double) r[c];
        }
    }
  Q centre[C],out[C];
  load_pixel<Q,C>(src+((size_t) y*a.columns+x)*C,centre);
  const double g=BLEND ? perceptible_reciprocal(gamma) : 1.0;
#pragma unroll
  for (int c=0; c < C; c++)
    {
      if ((a.copy_mask >> c) & 1u)
        out[c]=centre[c];
      else if (BLEND && (c != C-1))
        out[c]=QuantumOps<Q>::clamp(g*pixel[c]);
      else
        out[c]=QuantumOps<Q>::clamp(pixel[c]);
    }
  store_pixel<Q,C>(static_cast<Q *>(a.dst)+((size_t) y*a.columns+x)*C,out);
}

MhStatus launch_motion_blur(const View &src,const View &dst,const double *kernel,size_t width,
  const ptrdiff_t *offsets_xy,const Roles &roles)
{
  if ((width == 0) || (width > 65536))
    return fail(MH_BAD_ARGUMENT,"motion blur: bad kernel width");
  if (roles.blend && (roles.alpha != src.channels-1))
    return fail(MH_UNSUPPORTED,"alpha channel must be the last channel");
  std::vector<int> off(2*width);
  for (size_t j=0; j < 2*width; j++)
    off[j]=(int) offsets_xy[j];
  Temp d_kernel,d_offset;
  MH_TRY(upload_table(d_kernel,src.device,src.stream,kernel,width*sizeof(double)));
  MH_TRY(upload_table(d_offset,src.device,src.stream,off.data(),off.size()*sizeof(int)));
  MotionArgs a;
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.columns=(int) src.columns;
  a.rows=(int) src.rows;
  a.width=(int) width;
  a.kernel=d_kernel.as<double>();
  a.offset=d_offset.as<int>();
  a.copy_mask=roles.copy_mask;
  a.alpha=roles.alpha;
  ProfileScope prof("motion_blur",src.stream);
  dispatch_layout_blend(src.quantum,src.channels,roles.blend,[&](auto L) {
    hipLaunchKernelGGL((motion_blur_kernel<typename decltype(L)::Q,L.C,L.BLEND>),column_grid(a.columns,a.rows),
      dim3(kColumnBlock),0,src.stream,a); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ---------------------------------------------------------------- RotationalBlurImage
// effect.c:3209-3430: every pixel is the (alpha-weighted) mean of samples on the arc through it
// around the image centre; the sample stride grows towards the centre.  cos/sin tables come
// from the host (libm, as the reference); the coordinate expressions, the (ssize_t) casts and
// the accumulation order are the reference's.
struct RotationalArgs
{
  const void *src;
  void *dst;
  int columns,rows;
  int n;
  const double *cos_theta,*sin_theta;
  double center_x,center_y,blur_radius;
  uint32_t copy_mask;
  int has_alpha;               // the image has an alpha channel (last channel)
};

template<typename Q,int C>
__global__ __launch_bounds__(256)
void rotational_blur_kernel(RotationalArgs a)
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x),y=(int) blockIdx.y;
  if (x >= a.columns)
    return;
  const Q *src=static_cast<const Q *>(a.src);
  const double cx=(double) x-a.center_x,cy=(double) y-a.center_y;
  // hypot of two half-integers: x*x+y*y is exact in fp64, so sqrt is the correctly rounded hypot
  const double radius=sqrt(cx*cx+cy*cy);
  size_t step=1;
  if (radius != 0)
    {
      step=(size_t) (a.blur_radius/radius);
      if (step == 0)
        step=1;
      else if (step >= (size_t) a.n)
        step=(size_t) a.n-1;
    }
  double plain[C],weighted[C],gamma_plain=0.0,gamma_alpha=0.0;
#pragma unroll
  for (int c=0; c < C; c++)
    {
      plain[c]=0.0;
      weighted[c]=0.0;
    }
  for (size_t j=0; j < (size_t) a.n; j+=step)
    {
      long sx=(long) (a.center_x+cx*a.cos_theta[j]-cy*a.sin_theta[j]+0.5);
      long sy=(long) (a.center_y+cx*a.sin_theta[j]+cy*a.cos_theta[j]+0.5);
      sx=sx < 0 ? 0 : (sx > a.columns-1 ? a.columns-1 : sx);      // cache.c:2663-2679
      sy=sy < 0 ? 0 : (sy > a.rows-1 ? a.rows-1 : sy);
      Q r[C];
      load_pixel<Q,C>(src+((size_t) sy*a.columns+(size_t) sx)*C,r);
      const double alpha=a.has_alpha ? kQS*(double) r[C-1] : 1.0;
#pragma unroll
      for (int c=0; c < C; c++)
        {
          plain[c]+=(double) r[c];
          weighted[c]+=alpha*(double) r[c];
        }
      gamma_plain+=1.0;
      gamma_alpha+=alpha;
    }
  Q centre[C],out[C];
  load_pixel<Q,C>(src+((size_t) y*a.columns+x)*C,centre);
  const double gp=perceptible_reciprocal(gamma_plain),ga=perceptible_reciprocal(gamma_alpha);
#pragma unroll
  for (int c=0; c < C; c++)
    {
      if ((a.copy_mask >> c) & 1u)
        out[c]=centre[c];
      else if (!a.has_alpha || (c == C-1))
        out[c]=QuantumOps<Q>::clamp(gp*plain[c]);
      else
        out[c]=QuantumOps<Q>::clamp(ga*weighted[c]);
    }
  store_pixel<Q,C>(static_cast<Q *>(a.dst)+((size_t) y*a.columns+x)*C,out);
}

MhStatus launch_rotational_blur(const View &src,const View &dst,const double *cos_theta,
  const double *sin_theta,size_t n,double blur_radius,const Roles &roles)
{
  Temp d_cos,d_sin;
  MH_TRY(upload_table(d_cos,src.device,src.stream,cos_theta,n*sizeof(double)));
  MH_TRY(upload_table(d_sin,src.device,src.stream,sin_theta,n*sizeof(double)));
  RotationalArgs a;
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.columns=(int) src.columns;
  a.rows=(int) src.rows;
  a.n=(int) n;
  a.cos_theta=d_cos.as<double>();
  a.sin_theta=d_sin.as<double>();
  a.center_x=(double) (src.columns-1)/2.0;
  a.center_y=(double) (src.rows-1)/2.0;
  a.blur_radius=blur_radius;
  a.copy_mask=roles.copy_mask;
  a.has_alpha=roles.alpha >= 0 ? 1 : 0;
  if ((roles.alpha >= 0) && (roles.alpha != src.channels-1))
    return fail(MH_UNSUPPORTED,"alpha channel must be the last channel");
  ProfileScope prof("rotational_blur",src.stream);
  dispatch_layout(src.quantum,src.channels,[&](auto L) {
    hipLaunchKernelGGL((rotational_blur_kernel<typename decltype(L)::Q,L.C>),column_grid(a.columns,a.rows),
      dim3(kColumnBlock),0,src.stream,a); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ---------------------------------------------------------------- LocalContrastImage
// effect.c:1760-2010, literally: a vertical then a horizontal pass of the same (lopsided)
// triangular weighting — weights 1..w on the first w samples, then w+1, w, ..., 3 on the
// next w-1 — over the float luma, with a float intermediate image of columns+2w whose
// padding mirrors the neighbouring columns; then R,G,B are scaled by
// (luma + (luma-blurred)*strength/100)/luma.
struct LocalContrastArgs
{
  const void *src;
  void *dst;
  float *inter;                // rows x (columns+2w)
  int columns,rows,channels,w;
  double total_weight,strength_scale;
  uint32_t copy_mask;
  int colour;                  // 3 for R,G,B[,A], 1 for gray[,A]
};

template<typename Q>
static __device__ __forceinline__ float luma_of(const Q *p,int colour)
{
  // GetPixelLuma, pixel-accessor.h:304-315, narrowed to float as the scanline buffer does
  const double r=(double) p[0],g=(double) p[colour >= 3 ? 1 : 0],b=(double) p[colour >= 3 ? 2 : 0];
  return (float) (0.212656*r+0.715158*g+0.072186*b);
}

static __device__ __forceinline__ double lopsided_sum(const float *pix,long stride,int w)
{
  double weight=1.0,sum=0;
  for (int i=0; i < w; i++)
    {
      sum+=weight*((double) *pix);
      pix+=stride;
      weight+=1.0;
    }
  for (int i=w+1; i < (2*w); i++)
    {
      sum+=weight*((double) *pix);
      pix+=stride;
      weight-=1.0;
    }
  return sum;
}

template<typename Q>
__global__ __launch_bounds__(256)
void local_contrast_luma_kernel(LocalContrastArgs a,float *luma)       // luma: (rows+2w) x columns
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x),yy=(int) blockIdx.y;
  if (x >= a.columns)
    return;
  int y=yy-a.w;
  y=y < 0 ? 0 : (y > a.rows-1 ? a.rows-1 : y);                        // cache.c:2663-2679
  luma[(size_t) yy*a.columns+x]=luma_of<Q>(static_cast<const Q *>(a.src)+((size_t) y*a.columns+x)*a.channels,a.colour);
}

__global__ __launch_bounds__(256)
void local_contrast_vertical_kernel(LocalContrastArgs a,const float *luma)
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x),y=(int) blockIdx.y;
  if (x >= a.columns)
    return;
  const size_t pitch=(size_t) a.columns+2*(size_t) a.w;
  const double sum=lopsided_sum(luma+(size_t) y*a.columns+x,a.columns,a.w);
  float *out=a.inter+(size_t) y*pitch+(size_t) x+(size_t) a.w;
  const float value=(float) (sum/a.total_weight);
  *out=value;
  if ((x <= a.w) && (x != 0))                                          // mirror into the padding
    *(out-(x*2))=value;
  if ((x > a.columns-a.w-2) && (x != a.columns-1))
    *(out+((size_t) (a.columns-x-1)*2))=value;
}

template<typename Q>
__global__ __launch_bounds__(256)
void local_contrast_horizontal_kernel(LocalContrastArgs a)
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x),y=(int) blockIdx.y;
  if (x >= a.columns)
    return;
  const size_t pitch=(size_t) a.columns+2*(size_t) a.w;
  const double sum=lopsided_sum(a.inter+(size_t) y*pitch+x,1,a.w);
  const Q *p=static_cast<const Q *>(a.src)+((size_t) y*a.columns+x)*a.channels;
  Q *q=static_cast<Q *>(a.dst)+((size_t) y*a.columns+x)*a.channels;
  const double src_val=(double) luma_of<Q>(p,a.colour);
  double mult=(src_val-(sum/a.total_weight))*a.strength_scale;
  mult=(src_val+mult)/src_val;
  for (int c=0; c < a.channels; c++)
    {
      const bool colour_channel=c < a.colour;
      if (colour_channel && (((a.copy_mask >> c) & 1u) == 0))
        q[c]=QuantumOps<Q>::clamp((double) p[c]*mult);
      else
        q[c]=p[c];
    }
}

MhStatus launch_local_contrast(const View &src,const View &dst,double radius,double strength,
  const Roles &roles)
{
  LocalContrastArgs a;
  a.src=src.pixels;
  a.dst=dst.pixels;
  a.columns=(int) src.columns;
  a.rows=(int) src.rows;
  a.channels=src.channels;
  const long longest=(long) (src.columns > src.rows ? src.columns : src.rows);
  a.w=(int) (long) ((double) longest*0.002*fabs(radius));
  if ((a.w < 1) || (a.columns <= 2*a.w+2))
    return fail(MH_UNSUPPORTED,"LocalContrastImage: blur width %d on %d columns is left to the CPU",
      a.w,a.columns);
  a.total_weight=(double) (float) ((a.w+1)*(a.w+1));
  a.strength_scale=strength/100.0;
  a.copy_mask=roles.copy_mask;
  a.colour=src.channels-(roles.alpha >= 0 ? 1 : 0) >= 3 ? 3 : 1;
  Temp inter,luma;
  MH_TRY(inter.alloc(src.device,(size_t) a.rows*((size_t) a.columns+2*(size_t) a.w)*sizeof(float),src.stream));
  MH_TRY(luma.alloc(src.device,((size_t) a.rows+2*(size_t) a.w)*(size_t) a.columns*sizeof(float),src.stream));
  a.inter=inter.as<float>();
  const dim3 block(kColumnBlock),grid=column_grid(a.columns,a.rows);
  ProfileScope prof("local_contrast",src.stream);
  dispatch_quantum(src.quantum,[&](auto q) {
    hipLaunchKernelGGL((local_contrast_luma_kernel<decltype(q)>),column_grid(a.columns,a.rows+2*a.w),block,0,src.stream,a,
      luma.as<float>());
    hipLaunchKernelGGL(local_contrast_vertical_kernel,grid,block,0,src.stream,a,luma.as<float>());
    hipLaunchKernelGGL((local_contrast_horizontal_kernel<decltype(q)>),grid,block,0,src.stream,a); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ---------------------------------------------------------------- DespeckleImage
// effect.c:1211-1306 (Hull) and :1308-1490: per channel, 16 Hull calls (4 directions x
// {+,-} offset x {raise, lower}), each two data-parallel sweeps between two zero-bordered
// (columns+2) x (rows+2) planes.  All channels are swept together (they never interact);
// the step is ScaleCharToQuantum(1) = 257, the guard ScaleCharToQuantum(2) = 514.
template<typename Q,int C>
__global__ __launch_bounds__(256)
void despeckle_load_kernel(const Q *src,Q *f,Q *g,int columns,int rows)
{
  const int px=(int) (blockIdx.x*blockDim.x+threadIdx.x),py=(int) blockIdx.y;     // padded coordinates
  if (px >= columns+2)
    return;
  Q v[C];
#pragma unroll
  for (int c=0; c < C; c++)
    v[c]=(Q) 0;
  Q zero[C];
#pragma unroll
  for (int c=0; c < C; c++)
    zero[c]=(Q) 0;
  if ((px >= 1) && (px <= columns) && (py >= 1) && (py <= rows))
    load_pixel<Q,C>(src+((size_t) (py-1)*columns+(px-1))*C,v);
  store_pixel<Q,C>(f+((size_t) py*(columns+2)+px)*C,v);
  store_pixel<Q,C>(g+((size_t) py*(columns+2)+px)*C,zero);
}

// SECOND=false: g = f raised/lowered where the neighbour at +offset in f calls for it;
// SECOND=true:  f = g raised/lowered where the neighbours at -offset and +offset in g do
template<typename Q,int C,bool SECOND>
__global__ __launch_bounds__(256)
void hull_kernel(const Q *from,Q *to,int columns,int rows,int offset,int polarity)
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x),y=(int) blockIdx.y;
  if (x >= columns)
    return;
  const size_t i=((size_t) (y+1)*(columns+2)+(size_t) (x+1));
  Q centre[C],r[C],s[C],out[C];
  load_pixel<Q,C>(from+i*C,centre);
  load_pixel<Q,C>(from+(size_t) ((long) i+offset)*C,r);
  if (SECOND)
    load_pixel<Q,C>(from+(size_t) ((long) i-offset)*C,s);
#pragma unroll
  for (int c=0; c < C; c++)
    {
      double v=(double) centre[c];
      if (polarity > 0)
        {
          if (SECOND ? (((double) s[c] >= (v+514.0)) && ((double) r[c] > v)) : ((double) r[c] >= (v+514.0)))
            v+=257.0;
        }
      else
        {
          if (SECOND ? (((double) s[c] <= (v-514.0)) && ((double) r[c] < v)) : ((double) r[c] <= (v-514.0)))
            v-=257.0;
        }
      out[c]=(Q) v;
    }
  store_pixel<Q,C>(to+i*C,out);
}

template<typename Q,int C>
__global__ __launch_bounds__(256)
void despeckle_store_kernel(const Q *f,const Q *src,Q *dst,int columns,int rows,uint32_t copy_mask)
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x),y=(int) blockIdx.y;
  if (x >= columns)
    return;
  Q v[C],original[C];
  load_pixel<Q,C>(f+((size_t) (y+1)*(columns+2)+(x+1))*C,v);
  load_pixel<Q,C>(src+((size_t) y*columns+x)*C,original);
#pragma unroll
  for (int c=0; c < C; c++)
    if ((copy_mask >> c) & 1u)
      v[c]=original[c];
  store_pixel<Q,C>(dst+((size_t) y*columns+x)*C,v);
}

template<typename Q,int C>
static MhStatus despeckle_typed(const View &src,const View &dst,const Roles &roles)
{
  const int W=(int) src.columns,H=(int) src.rows;
  const size_t plane=(size_t) (W+2)*(size_t) (H+2)*C*sizeof(Q);
  Temp tf,tg;
  MH_TRY(tf.alloc(src.device,plane,src.stream));
  MH_TRY(tg.alloc(src.device,plane,src.stream));
  Q *f=tf.as<Q>(),*g=tg.as<Q>();
  const dim3 block(kColumnBlock);
  ProfileScope prof("despeckle",src.stream);
  hipLaunchKernelGGL((despeckle_load_kernel<Q,C>),column_grid(W+2,H+2),block,0,
    src.stream,static_cast<const Q *>(src.pixels),f,g,W,H);
  const dim3 grid=column_grid(W,H);
  static const int X[4]={0,1,1,-1},Y[4]={1,0,1,1};
  for (int k=0; k < 4; k++)
    {
      const int offset=Y[k]*(W+2)+X[k];
      const int sequence[4][2]={{offset,1},{-offset,1},{-offset,-1},{offset,-1}};
      for (const auto &call : sequence)
        {
          hipLaunchKernelGGL((hull_kernel<Q,C,false>),grid,block,0,src.stream,f,g,W,H,call[0],call[1]);
          hipLaunchKernelGGL((hull_kernel<Q,C,true>),grid,block,0,src.stream,g,f,W,H,call[0],call[1]);
        }
    }
  hipLaunchKernelGGL((despeckle_store_kernel<Q,C>),grid,block,0,src.stream,f,static_cast<const Q *>(src.pixels),
    static_cast<Q *>(dst.pixels),W,H,roles.copy_mask);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_despeckle(const View &src,const View &dst,const Roles &roles)
{
  return dispatch_layout(src.quantum,src.channels,[&](auto L) {
    return despeckle_typed<typename decltype(L)::Q,L.C>(src,dst,roles); });
}

// ---------------------------------------------------------------- WaveletDenoiseImage
// visual-effects.c:3478-3760: five levels of the a-trous "hat" transform (rows, then columns)
// on float planes of the colour channels, soft thresholding of each detail band, and the
// reconstruction.  All arithmetic is the reference's float arithmetic, expression by
// expression (HatTransform's three index ranges in closed form).
static __device__ __forceinline__ float hat_value(const float *line,long stride,int i,int extent,int scale)
{
  const float centre=line[(long) i*stride];
  if (i < scale)
    return 0.25f*(centre+centre+line[(long) (scale-i)*stride]+line[(long) (scale+i)*stride]);
  if (i < extent-scale)
    return 0.25f*(2.0f*centre+line[(long) (i-scale)*stride]+line[(long) (i+scale)*stride]);
  return 0.25f*(centre+centre+line[(long) (i-scale)*stride]+line[(long) (2*extent-2-scale-i)*stride]);
}

template<typename Q>
__global__ __launch_bounds__(256)
void wavelet_load_kernel(const Q *src,float *plane,size_t npixels,int channels,int colour)
{
  const size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x;
  if (i >= npixels)
    return;
  for (int c=0; c < colour; c++)
    plane[i*colour+c]=(float) src[i*channels+c];
}

// ROWS: out(x,y) from the row y of `in`; else from the column x
template<bool ROWS>
__global__ __launch_bounds__(256)
void wavelet_hat_kernel(const float *in,float *out,int columns,int rows,int colour,int scale)
{
  const int xc=(int) (blockIdx.x*blockDim.x+threadIdx.x),y=(int) blockIdx.y;     // xc = x*colour+c
  if (xc >= columns*colour)
    return;
  const int x=xc/colour,c=xc-x*colour;
  const size_t pitch=(size_t) columns*colour;
  float v;
  if (ROWS)
    v=hat_value(in+(size_t) y*pitch+c,colour,x,columns,scale);
  else
    v=hat_value(in+(size_t) x*colour+c,(long) pitch,y,rows,scale);
  out[(size_t) y*pitch+xc]=v;
}

__global__ __launch_bounds__(256)
void wavelet_threshold_kernel(float *high,const float *low,float *base,size_t count,double magnitude,
  double softness,int accumulate)
{
  const size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x;
  if (i >= count)
    return;
  float h=high[i];
  h-=low[i];
  if ((double) h < -magnitude)
    h+=(float) (magnitude-softness*magnitude);
  else if ((double) h > magnitude)
    h-=(float) (magnitude-softness*magnitude);
  else
    h*=(float) softness;
  high[i]=h;
  if (accumulate != 0)
    base[i]+=h;
}

template<typename Q>
__global__ __launch_bounds__(256)
void wavelet_store_kernel(const Q *src,Q *dst,const float *base,const float *low,size_t npixels,int channels,
  int colour,uint32_t copy_mask)
{
  const size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x;
  if (i >= npixels)
    return;
  for (int c=0; c < channels; c++)
    {
      // every colour channel is rebuilt, whatever its traits (visual-effects.c:3590-3598 only
      // skips channels that are not R, G or B)
      if (c < colour)
        dst[i*channels+c]=QuantumOps<Q>::clamp((double) base[i*colour+c]+(double) low[i*colour+c]);
      else
        dst[i*channels+c]=src[i*channels+c];
    }
}

MhStatus launch_wavelet_denoise(const View &src,const View &dst,double threshold,double softness,
  const Roles &roles)
{
  const int W=(int) src.columns,H=(int) src.rows;
  if ((W < 33) || (H < 33))
    return fail(MH_UNSUPPORTED,"WaveletDenoiseImage: %dx%d is below two spans of the coarsest level",W,H);
  const int colour=src.channels-(roles.alpha >= 0 ? 1 : 0) >= 3 ? 3 : 1;
  const size_t n=(size_t) W*H,count=n*(size_t) colour;
  Temp planes[4];
  float *plane[4];
  for (int k=0; k < 4; k++)
    {
      MH_TRY(planes[k].alloc(src.device,count*sizeof(float),src.stream));
      plane[k]=planes[k].as<float>();
    }
  static const float noise_levels[]={0.8002f,0.2735f,0.1202f,0.0585f,0.0291f,0.0152f,0.0080f,0.0044f};
  const dim3 block(kColumnBlock);
  const dim3 pixel_blocks=column_grid(n),value_blocks=column_grid(count);
  ProfileScope prof("wavelet_denoise",src.stream);
  dispatch_quantum(src.quantum,[&](auto q) {
    using Q=decltype(q);
    hipLaunchKernelGGL((wavelet_load_kernel<Q>),pixel_blocks,block,0,src.stream,
      static_cast<const Q *>(src.pixels),plane[0],n,src.channels,colour); });
  const dim3 grid=column_grid(W*colour,H);
  int high=0,low=1;
  for (int level=0; level < 5; level++)
    {
      low=(level & 1)+1;                             // low_pass = number_pixels*((level & 0x01)+1)
      hipLaunchKernelGGL((wavelet_hat_kernel<true>),grid,block,0,src.stream,plane[high],plane[3],W,H,colour,
        1 << level);
      hipLaunchKernelGGL((wavelet_hat_kernel<false>),grid,block,0,src.stream,plane[3],plane[low],W,H,colour,
        1 << level);
      const double magnitude=threshold*(double) noise_levels[level];
      hipLaunchKernelGGL(wavelet_threshold_kernel,value_blocks,block,0,src.stream,plane[high],plane[low],
        plane[0],count,magnitude,softness,high != 0 ? 1 : 0);
      high=low;
    }
  dispatch_quantum(src.quantum,[&](auto q) {
    using Q=decltype(q);
    hipLaunchKernelGGL((wavelet_store_kernel<Q>),pixel_blocks,block,0,src.stream,
      static_cast<const Q *>(src.pixels),static_cast<Q *>(dst.pixels),plane[0],plane[low],n,
      src.channels,colour,roles.copy_mask); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

} // namespace mh
