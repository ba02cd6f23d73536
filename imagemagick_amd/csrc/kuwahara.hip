// KuwaharaImage (MagickCore/effect.c:1775-1978) behind its BlurImage: the selection of the calmest
// quadrant and the interpolated copy, bit-identical to the reference in both precision modes, Q16
// and float Quantum, 1-4 channels.  The frame this kernel reads is the BLURRED one (the caller runs
// the bit-identical BlurImage first, operators.cpp); the reference reads nothing else either.
//
//   w = (size_t) radius + 1.  For the output pixel (x,y) four w x w windows of the blurred frame,
//   origins (x-(w-1),y-(w-1)), (x,y-(w-1)), (x-(w-1),y), (x,y), edge-clamped.  Per window: the mean of
//   every channel (a sequential fp64 sum in raster order, divided by (double) (w*w)), the mean luma
//   0.212656*mR+0.715158*mG+0.072186*mB, and the variance, the sequential sum of
//   (luma-mean_luma)*(luma-mean_luma) with luma the same expression on the samples (on a gray
//   layout R, G and B all live at offset 0 and the expression is kept as written).  The first
//   window with the strictly smallest variance wins, and the output pixel is the bilinear branch of
//   InterpolatePixelChannels (pixel.c:4975-5033) at (origin.x+w/2.0, origin.y+w/2.0): all channels,
//   those whose trait carries Blend weighted by alpha.  No channel is copied from the source.
//
// MI355X mapping, edge_blur.hip's: a workgroup of 256 lanes computes a
// 16 x 16 block of outputs and stages the block's edge-clamped window in LDS once: w-1 pixels to
// the left and above, max(w-1,w/2+1) to the right and below (the 2 x 2 fetch of the interpolation
// reaches one pixel past the windows for w <= 2), one plane per channel of raw samples plus one
// plane of fp64 lumas.  Quadrant 3 of (x,y) is quadrant 0 of (x+w-1,y+w-1): the block has only
// (15+w)^2 distinct windows, not 4*256.  Phase 1: the lanes share those windows out and walk each
// once, in the reference's order, every multiply and add separately rounded (-ffp-contract=off),
// into an LDS map of variances.  Phase 2, behind one barrier: every lane compares its four map
// entries in quadrant order and interpolates from the staged samples.
//
// Limit: planes and map must fit kKuwaharaMaxLds = 128 KiB of LDS; larger windows return
// MH_UNSUPPORTED.  A staged pixel costs channels*sizeof(Quantum)+8 bytes, a window 8.  RGBA float
// Quantum, the dearest case, fits w <= 27 (every radius below 27), RGBA Q16 w <= 34, gray Q16
// w <= 43.  NaN and infinite samples are out of scope.
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"

#include <algorithm>

namespace mh {

constexpr int kKuwaharaBlock=kWindowBlock;       // outputs per workgroup: kKuwaharaBlock x kKuwaharaBlock
constexpr size_t kKuwaharaMaxLds=131072;         // bytes of the staged planes and the variance map

struct KuwaharaArgs
{
  const void *blurred;       // BlurImage(image,radius,sigma)
  const void *original;      // image: read only where keep_mask is set
  void *dst;
  int columns,rows;
  int width;                 // w
  int tile;                  // side of the staged window: kKuwaharaBlock+(w-1)+max(w-1,w/2+1)
  int pitch;                 // row pitch of every staged plane, in elements
  int map;                   // distinct windows per side: kKuwaharaBlock+w-1
  uint32_t blend_mask;       // channels whose trait carries Blend
  uint32_t keep_mask;        // channels with an undefined trait: InterpolatePixelChannels skips them
  int alpha;                 // the channel GetPixelAlpha reads, -1: OpaqueAlpha
  int gray;                  // R, G and B all live at offset 0
};

// GetPixelLuma / GetMeanLuma, pixel-accessor.h:304-315 and effect.c:1767-1773
static __device__ __forceinline__ double kuwahara_luma(double red,double green,double blue)
{
  return 0.212656*red+0.715158*green+0.072186*blue;
}

template<typename Q,int C>
__global__ __launch_bounds__(256)
void kuwahara_kernel(KuwaharaArgs a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char kuwahara_smem[];
  constexpr int L=C >= 3 ? 3 : 1;          // planes the luma reads (a gray layout: the first one)
  constexpr int G=L == 3 ? 1 : 0,B=L == 3 ? 2 : 0;
  const int plane=a.tile*a.pitch;
  double *lumas=reinterpret_cast<double *>(kuwahara_smem);
  double *variances=lumas+plane;
  Q *samples=reinterpret_cast<Q *>(variances+a.map*a.map);
  const int tx=(int) (threadIdx.x % kKuwaharaBlock),ty=(int) (threadIdx.x/kKuwaharaBlock);
  const int x0=(int) blockIdx.x*kKuwaharaBlock,y0=(int) blockIdx.y*kKuwaharaBlock;
  const int x=x0+tx,y=y0+ty;
  const int w=a.width,reach=w-1;
  const bool gray=(L == 1) || (a.gray != 0);
  for (int i=(int) threadIdx.x; i < a.tile*a.tile; i+=(int) blockDim.x)
    {
      const int r=i/a.tile,col=i-r*a.tile;
      const int gx=min(max(x0-reach+col,0),a.columns-1),gy=min(max(y0-reach+r,0),a.rows-1);
      Q q[C];
      load_pixel<Q,C>(static_cast<const Q *>(a.blurred)+((size_t) gy*(size_t) a.columns+(size_t) gx)*C,q);
      const int cell=r*a.pitch+col;
#pragma unroll
      for (int c=0; c < C; c++)
        samples[c*plane+cell]=q[c];
      const double red=(double) q[0];
      lumas[cell]=kuwahara_luma(red,gray ? red : (double) q[G],gray ? red : (double) q[B]);
    }
  __syncthreads();
  // phase 1: window (mx,my) of the map has its origin at tile cell (mx,my); the windows that only
  // pixels outside the frame would ask for are left out
  const int need_x=min(kKuwaharaBlock,a.columns-x0)+reach,need_y=min(kKuwaharaBlock,a.rows-y0)+reach;
  const double count=(double) ((size_t) w*(size_t) w);
  for (int i=(int) threadIdx.x; i < a.map*a.map; i+=(int) blockDim.x)
    {
      const int my=i/a.map,mx=i-my*a.map;
      if ((mx >= need_x) || (my >= need_y))
        continue;
      double mean[L];
#pragma unroll
      for (int c=0; c < L; c++)
        mean[c]=0.0;
      for (int v=0; v < w; v++)
        {
          const int row=(my+v)*a.pitch+mx;
          for (int u=0; u < w; u++)
            {
#pragma unroll
              for (int c=0; c < L; c++)
                mean[c]+=(double) samples[c*plane+row+u];
            }
        }
#pragma unroll
      for (int c=0; c < L; c++)
        mean[c]/=count;
      const double mean_luma=kuwahara_luma(mean[0],gray ? mean[0] : mean[G],gray ? mean[0] : mean[B]);
      double variance=0.0;
      for (int v=0; v < w; v++)
        {
          const int row=(my+v)*a.pitch+mx;
          for (int u=0; u < w; u++)
            {
              const double d=lumas[row+u]-mean_luma;
              variance+=d*d;
            }
        }
      variances[i]=variance;
    }
  __syncthreads();
  if ((x >= a.columns) || (y >= a.rows))
    return;
  // phase 2: strict <, so a tie keeps the earliest quadrant (effect.c:1938-1942)
  int best_x=tx,best_y=ty;
  double min_variance=variances[ty*a.map+tx];
  {
    double variance=variances[ty*a.map+tx+reach];
    if (variance < min_variance)
      {
        min_variance=variance;
        best_x=tx+reach;
        best_y=ty;
      }
    variance=variances[(ty+reach)*a.map+tx];
    if (variance < min_variance)
      {
        min_variance=variance;
        best_x=tx;
        best_y=ty+reach;
      }
    variance=variances[(ty+reach)*a.map+tx+reach];
    if (variance < min_variance)
      {
        best_x=tx+reach;
        best_y=ty+reach;
      }
  }
  // InterpolatePixelChannels at (origin+w/2.0): the 2 x 2 block from floor(), delta = 0 or 0.5
  const int half=w/2;
  const double delta=0.5*(double) (w & 1),epsilon=1.0-delta;
  const int p0=(best_y+half)*a.pitch+best_x+half,p1=p0+1,p2=p0+a.pitch,p3=p2+1;
  const double opaque=kQS*65535.0;
  const double alpha0=a.alpha >= 0 ? kQS*(double) samples[a.alpha*plane+p0] : opaque;
  const double alpha1=a.alpha >= 0 ? kQS*(double) samples[a.alpha*plane+p1] : opaque;
  const double alpha2=a.alpha >= 0 ? kQS*(double) samples[a.alpha*plane+p2] : opaque;
  const double alpha3=a.alpha >= 0 ? kQS*(double) samples[a.alpha*plane+p3] : opaque;
  Q out[C];
  if (a.keep_mask != 0u)
    load_pixel<Q,C>(static_cast<const Q *>(a.original)+((size_t) y*(size_t) a.columns+(size_t) x)*C,out);
#pragma unroll
  for (int c=0; c < C; c++)
    {
      if ((a.keep_mask >> c) & 1u)
        continue;
      double pixel0=(double) samples[c*plane+p0],pixel1=(double) samples[c*plane+p1];
      double pixel2=(double) samples[c*plane+p2],pixel3=(double) samples[c*plane+p3];
      double gamma;
      if ((a.blend_mask >> c) & 1u)
        {
          pixel0*=alpha0;
          pixel1*=alpha1;
          pixel2*=alpha2;
          pixel3*=alpha3;
          gamma=epsilon*(epsilon*alpha0+delta*alpha1)+delta*(epsilon*alpha2+delta*alpha3);
        }
      else
        gamma=epsilon*(epsilon+delta)+delta*(epsilon+delta);
      gamma=perceptible_reciprocal(gamma);
      out[c]=QuantumOps<Q>::clamp(gamma*(epsilon*(epsilon*pixel0+delta*pixel1)+delta*(epsilon*pixel2+
        delta*pixel3)));
    }
  store_pixel<Q,C>(static_cast<Q *>(a.dst)+((size_t) y*(size_t) a.columns+(size_t) x)*C,out);
}

// Row pitch of the staged planes.  Phase 1 gives consecutive windows to consecutive lanes, and a
// row of the map has `map` windows, so a pitch of map (mod 32) elements lets the lanes of a wave
// that straddle two map rows go on reading consecutive LDS banks.  The padding is dropped when
// only the plain pitch fits the budget.
static bool kuwahara_layout(size_t w,int channels,size_t sample,KuwaharaArgs *a,size_t *lds)
{
  const size_t reach=w-1,tile=kKuwaharaBlock+reach+std::max<size_t>(reach,w/2+1),map=kKuwaharaBlock+reach;
  const size_t pixel=(size_t) channels*sample+sizeof(double);
  size_t pitch=tile+((map+32u-(tile & 31u)) & 31u);
  if (map*map*sizeof(double)+pitch*tile*pixel > kKuwaharaMaxLds)
    pitch=(tile+3u) & ~(size_t) 3u;
  const size_t bytes=map*map*sizeof(double)+pitch*tile*pixel;
  if (bytes > kKuwaharaMaxLds)
    return false;
  a->width=(int) w;
  a->tile=(int) tile;
  a->pitch=(int) pitch;
  a->map=(int) map;
  *lds=(bytes+15u) & ~(size_t) 15u;
  return true;
}

static MhStatus kuwahara_plan(const View &src,double radius,KuwaharaArgs *a,size_t *lds)
{
  // width=(size_t) radius+1 (effect.c:1809)
  if (!(radius >= 0.0) || (radius > 4096.0))
    return fail(MH_UNSUPPORTED,"KuwaharaImage: radius %g does not fit the LDS tile",radius);
  const size_t w=(size_t) radius+1;
  if ((src.channels < 1) || (src.channels > 4))
    return fail(MH_UNSUPPORTED,"KuwaharaImage: %d channels",src.channels);
  MH_TRY(window_grid_check("KuwaharaImage",src));
  if (!kuwahara_layout(w,src.channels,src.quantum == MH_QUANTUM_U16 ? 2u : 4u,a,lds) ||
      (*lds > (size_t) lds_bytes_per_workgroup(src.device)))
    return fail(MH_UNSUPPORTED,"KuwaharaImage: a %zux%zu window does not fit the LDS tile",w,w);
  return MH_OK;
}

MhStatus kuwahara_check(const View &src,double radius)
{
  KuwaharaArgs a={};
  size_t lds=0;
  return kuwahara_plan(src,radius,&a,&lds);
}

template<typename Q,int C>
static MhStatus kuwahara_launch(const KuwaharaArgs &a,size_t lds,hipStream_t stream)
{
  MH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&kuwahara_kernel<Q,C>),
    hipFuncAttributeMaxDynamicSharedMemorySize,(int) kKuwaharaMaxLds));
  ProfileScope prof("kuwahara",stream);
  hipLaunchKernelGGL((kuwahara_kernel<Q,C>),window_grid(a.columns,a.rows),dim3(kKuwaharaBlock*kKuwaharaBlock),lds,stream,a);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_kuwahara(const View &blurred,const View &original,const View &dst,double radius,
  const MhImage *image,const MhImage *kuwahara_image)
{
  KuwaharaArgs a={};
  size_t lds=0;
  MH_TRY(kuwahara_plan(blurred,radius,&a,&lds));
  if ((blurred.columns == 0) || (blurred.rows == 0))
    return MH_OK;
  a.blurred=blurred.pixels;
  a.original=original.pixels;
  a.dst=dst.pixels;
  a.columns=(int) blurred.columns;
  a.rows=(int) blurred.rows;
  // the traits of the blurred frame are the source's (BlurImage clones it), those of the
  // destination the result's (pixel.c:4990-5005)
  for (int c=0; c < blurred.channels; c++)
    {
      if ((image->channel_traits[c] == MH_TRAIT_UNDEFINED) || (kuwahara_image->channel_traits[c] == MH_TRAIT_UNDEFINED))
        a.keep_mask|=1u << c;
      else if ((image->channel_traits[c] & MH_TRAIT_BLEND) != 0)
        a.blend_mask|=1u << c;
    }
  // GetPixelAlpha, pixel-accessor.h:59-65: OpaqueAlpha unless the alpha channel has a trait
  a.alpha=(image->alpha_offset >= 0) && (image->channel_traits[image->alpha_offset] != MH_TRAIT_UNDEFINED) ?
    image->alpha_offset : -1;
  a.gray=(image->colorspace == MH_COLORSPACE_GRAY) || (image->colorspace == MH_COLORSPACE_LINEARGRAY) ||
    (blurred.channels < 3);
  return dispatch_layout(blurred.quantum,blurred.channels,[&](auto L) {
    return kuwahara_launch<typename decltype(L)::Q,L.C>(a,lds,blurred.stream); });
}

} // namespace mh
