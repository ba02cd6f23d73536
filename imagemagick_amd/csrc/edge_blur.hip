// The two edge-preserving blurs of MagickCore/effect.c, bit-identical to the reference in both
// precision modes, Q16 and float Quantum, 1-4 channels:
//
//   BilateralBlurImage (effect.c:894-1142)   W x H window, W = max(width,1), H = max(height,1),
//     from (x-W/2, y-H/2), edge-clamped.  Tap n = v*W+u reads the pixel at (W/2-u, H/2-v) from the
//     centre (a reflected raster walk) and weighs it by
//       intensity_gaussian[char(tap) - char(centre) + 255] * spatial_gaussian[n]
//     where char() = ScaleQuantumToChar((Quantum) GetPixelIntensity()).
//   SelectiveBlurImage (effect.c:3406-3710)  width x width window, centred, edge-clamped, raster
//     order; a tap takes part when its contrast to the centre's intensity is below the threshold.
//     Blend channels measure the tap's own GetPixelIntensity; every other channel measures the
//     tap's pixel in the gray clone the reference makes with TransformImageColorspace.
//
// MI355X mapping, statistic.hip's: a workgroup of 256 lanes computes a
// 16 x 16 block of outputs.  It stages the block's (15+W) x (15+H) edge-clamped window in LDS once,
// one plane per channel of raw samples plus what the weights need (bilateral: one intensity byte a
// pixel and the 511-entry intensity Gaussian; selective: the intensity and the gray clone's
// intensity as doubles), then every lane walks its own window ONCE for all channels: a tap's
// weight is formed once and feeds one fp64 sum per channel, each sum in the reference's order,
// every multiply and add separately rounded (-ffp-contract=off).  The tables that every lane reads
// at the same index (spatial Gaussian, selective kernel) stay in global memory: the index is
// uniform, so they come through the scalar cache.  All transcendentals are evaluated on the host
// (kernel_info.cpp); no exp on the device.
//
// Limit: the staged tile must fit kEdgeMaxLds = 128 KiB of LDS (what a pixel costs is in
// launch_bilateral_blur / launch_selective_blur); larger windows return MH_UNSUPPORTED.  RGBA float
// Quantum, the dearest case, fits square windows up to 69 x 69 (bilateral) and 49 x 49 (selective).
//
// Declined (MH_UNSUPPORTED) on purpose: an even bilateral W or H - the reference's reflected walk
// then reads one column and one row past the window it fetched.  Restated differently on purpose:
// intensity_gaussian[510] (a difference of +255: white tap, black centre), which the reference
// never writes (its fill loop stops at w < 255) and reads from an uninitialised stack slot; here it
// is BlurGaussian(255, intensity_sigma).  NaN samples are out of scope for both operators.
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "pixel_intensity.hpp"

#include <algorithm>
#include <vector>

namespace mh {

constexpr int kEdgeBlock=kWindowBlock;       // outputs per workgroup: kEdgeBlock x kEdgeBlock
constexpr size_t kEdgeMaxLds=131072;         // bytes of the staged tile
constexpr int kIntensityTable=512;           // 2*(MaxIntensity+1) doubles, 511 of them used

// how the selective blur's gray clone comes about
enum { LUM_SELF=0,LUM_FROM_SRGB=1,LUM_FROM_LINEAR=2 };

struct EdgeArgs
{
  const void *src;
  void *dst;
  const double *tables;      // bilateral: intensity Gaussian [512], spatial Gaussian [W*H]; selective: kernel
  int columns,rows;
  int width,height;          // W, H: odd, >= 1
  int tile_w,tile_h;         // kEdgeBlock-1+W, kEdgeBlock-1+H
  int pitch;                 // row pitch of every staged plane, in elements
  uint32_t copy_mask;
  int alpha;                 // alpha channel when the colour channels blend, else -1
  int stage_intensity,stage_luminance;      // selective: which of the two fp64 planes are staged
  int luminance,luminance_channels;         // selective: LUM_*, channels of the gray clone
  double threshold;
  IntensityParams ip,luminance_ip;
};

// ScaleQuantumToChar((Quantum) intensity), quantum.h:113-124: the conversion to Quantum truncates
// on Q16 and rounds to float on float Quantum
template<typename Q>
static __device__ __forceinline__ unsigned char intensity_char(double intensity)
{
  if constexpr (QuantumOps<Q>::is_float)
    {
      const float q=(float) intensity;
      if (!(q > 0.0f))
        return 0;
      if ((q/257.0f) >= 255.0f)
        return 255;
      return (unsigned char) (q/257.0f+0.5f);
    }
  else
    {
      const unsigned long q=(unsigned long) (uint16_t) (int) intensity+128ul;
      return (unsigned char) ((q-(q >> 8)) >> 8);
    }
}

// the frame's pixel under tile cell i (edge-clamped)
template<typename Q,int C>
static __device__ __forceinline__ void edge_fetch(const EdgeArgs &a,int left,int top,int i,int &cell,Q (&q)[C])
{
  const int r=i/a.tile_w,col=i-r*a.tile_w;
  const int gx=min(max(left+col,0),a.columns-1),gy=min(max(top+r,0),a.rows-1);
  load_pixel<Q,C>(static_cast<const Q *>(a.src)+((size_t) gy*(size_t) a.columns+(size_t) gx)*C,q);
  cell=r*a.pitch+col;
}

template<typename Q,int C>
__global__ __launch_bounds__(256)
void bilateral_blur_kernel(EdgeArgs a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char edge_smem[];
  const int plane=a.tile_h*a.pitch;
  double *gaussian=reinterpret_cast<double *>(edge_smem);
  Q *samples=reinterpret_cast<Q *>(edge_smem+kIntensityTable*sizeof(double));
  unsigned char *keys=reinterpret_cast<unsigned char *>(samples+(size_t) C*plane);
  const int tx=(int) (threadIdx.x % kEdgeBlock),ty=(int) (threadIdx.x/kEdgeBlock);
  const int x0=(int) blockIdx.x*kEdgeBlock,y0=(int) blockIdx.y*kEdgeBlock;
  const int x=x0+tx,y=y0+ty;
  const bool inside=(x < a.columns) && (y < a.rows);
  const int mid_x=a.width/2,mid_y=a.height/2;
  for (int i=(int) threadIdx.x; i < kIntensityTable; i+=(int) blockDim.x)
    gaussian[i]=a.tables[i];
  for (int i=(int) threadIdx.x; i < a.tile_w*a.tile_h; i+=(int) blockDim.x)
    {
      Q q[C];
      int cell;
      edge_fetch<Q,C>(a,x0-mid_x,y0-mid_y,i,cell,q);
#pragma unroll
      for (int c=0; c < C; c++)
        samples[c*plane+cell]=q[c];
      keys[cell]=intensity_char<Q>(pixel_intensity<Q,C>(q,a.ip));
    }
  __syncthreads();
  if (!inside)
    return;
  const double *spatial=a.tables+kIntensityTable;
  const int centre=(ty+mid_y)*a.pitch+tx+mid_x;
  const int centre_key=(int) keys[centre]-255;
  const bool blend=a.alpha >= 0;
  const double alpha=blend ? kQS*(double) samples[a.alpha*plane+centre] : 0.0;
  double pixel[C],gamma=0.0,blend_gamma=0.0;
#pragma unroll
  for (int c=0; c < C; c++)
    pixel[c]=0.0;
  int n=0;
  for (int v=0; v < a.height; v++)
    {
      // tap (u,v) lies (mid_x-u, mid_y-v) from the centre: W-1-u, H-1-v from the window's corner
      const int row=(ty+a.height-1-v)*a.pitch+tx+a.width-1;
      for (int u=0; u < a.width; u++)
        {
          const int cell=row-u;
          const double weight=gaussian[(int) keys[cell]-centre_key]*spatial[n];
#pragma unroll
          for (int c=0; c < C; c++)
            pixel[c]+=weight*(double) samples[c*plane+cell];
          gamma+=weight;
          if (blend)
            blend_gamma+=weight*alpha*(kQS*(double) samples[a.alpha*plane+cell]);
          n++;
        }
    }
  Q out[C];
#pragma unroll
  for (int c=0; c < C; c++)
    {
      if ((a.copy_mask >> c) & 1u)
        out[c]=samples[c*plane+centre];
      else
        out[c]=QuantumOps<Q>::clamp(perceptible_reciprocal(blend && (c != a.alpha) ? blend_gamma : gamma)*pixel[c]);
    }
  store_pixel<Q,C>(static_cast<Q *>(a.dst)+((size_t) y*(size_t) a.columns+(size_t) x)*C,out);
}

// GetPixelIntensity of the pixel's counterpart in the gray clone (effect.c:3510-3517, :3629)
template<typename Q,int C>
static __device__ __forceinline__ double luminance_intensity(const Q (&q)[C],const EdgeArgs &a)
{
  if (a.luminance == LUM_SELF)
    return pixel_intensity<Q,C>(q,a.ip);          // a gray image is its own clone
  if constexpr (C >= 3)
    {
      double red=(double) q[0],green=(double) q[1],blue=(double) q[2];
      if (a.luminance == LUM_FROM_LINEAR)
        {
          // linear RGB -> sRGB, every channel stored as a Quantum (colorspace.c:2547-2552)
          red=(double) QuantumOps<Q>::clamp(encode_pixel_gamma(red));
          green=(double) QuantumOps<Q>::clamp(encode_pixel_gamma(green));
          blue=(double) QuantumOps<Q>::clamp(encode_pixel_gamma(blue));
        }
      // sRGB -> GRAY, stored as a Quantum (colorspace.c:943-945)
      const Q gray=QuantumOps<Q>::clamp(0.212656*red+0.715158*green+0.072186*blue);
      if (a.luminance_channels == 1)
        return (double) gray;
      const Q clone[2]={gray,q[C-1]};
      return pixel_intensity<Q,2>(clone,a.luminance_ip);
    }
  else
    return pixel_intensity<Q,C>(q,a.ip);
}

template<typename Q,int C>
__global__ __launch_bounds__(256)
void selective_blur_kernel(EdgeArgs a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char edge_smem[];
  const int plane=a.tile_h*a.pitch;
  double *intensities=reinterpret_cast<double *>(edge_smem);
  double *luminances=intensities+(a.stage_intensity ? plane : 0);
  Q *samples=reinterpret_cast<Q *>(luminances+(a.stage_luminance ? plane : 0));
  const int tx=(int) (threadIdx.x % kEdgeBlock),ty=(int) (threadIdx.x/kEdgeBlock);
  const int x0=(int) blockIdx.x*kEdgeBlock,y0=(int) blockIdx.y*kEdgeBlock;
  const int x=x0+tx,y=y0+ty;
  const bool inside=(x < a.columns) && (y < a.rows);
  const int mid=a.width/2;
  for (int i=(int) threadIdx.x; i < a.tile_w*a.tile_h; i+=(int) blockDim.x)
    {
      Q q[C];
      int cell;
      edge_fetch<Q,C>(a,x0-mid,y0-mid,i,cell,q);
#pragma unroll
      for (int c=0; c < C; c++)
        samples[c*plane+cell]=q[c];
      if (a.stage_intensity)
        intensities[cell]=pixel_intensity<Q,C>(q,a.ip);
      if (a.stage_luminance)
        luminances[cell]=luminance_intensity<Q,C>(q,a);
    }
  __syncthreads();
  if (!inside)
    return;
  Q out[C];
  load_pixel<Q,C>(static_cast<const Q *>(a.src)+((size_t) y*(size_t) a.columns+(size_t) x)*C,out);
  const double intensity=pixel_intensity<Q,C>(out,a.ip);
  const bool blend=a.alpha >= 0;
  // one gamma for the blend channels and one for the others: the same sum for each of them
  double pixel[C],blend_gamma=0.0,gamma=0.0;
#pragma unroll
  for (int c=0; c < C; c++)
    pixel[c]=0.0;
  int n=0;
  for (int v=0; v < a.width; v++)
    {
      const int row=(ty+v)*a.pitch+tx;
      for (int u=0; u < a.width; u++)
        {
          const int cell=row+u;
          const double k=a.tables[n];
          n++;
          if (blend && (fabs(intensities[cell]-intensity) < a.threshold))
            {
              const double weight=k*(kQS*(double) samples[a.alpha*plane+cell]);
#pragma unroll
              for (int c=0; c < C; c++)
                if (c != a.alpha)
                  pixel[c]+=weight*(double) samples[c*plane+cell];
              blend_gamma+=weight;
            }
          if (a.stage_luminance && (fabs(luminances[cell]-intensity) < a.threshold))
            {
#pragma unroll
              for (int c=0; c < C; c++)
                if (!blend || (c == a.alpha))
                  pixel[c]+=k*(double) samples[c*plane+cell];
              gamma+=k;
            }
        }
    }
#pragma unroll
  for (int c=0; c < C; c++)
    {
      if ((a.copy_mask >> c) & 1u)
        continue;                                   // out[c] is the centre sample
      const double g=blend && (c != a.alpha) ? blend_gamma : gamma;
      if (!(fabs(g) < kEps))
        out[c]=QuantumOps<Q>::clamp(perceptible_reciprocal(g)*pixel[c]);
    }
  store_pixel<Q,C>(static_cast<Q *>(a.dst)+((size_t) y*(size_t) a.columns+(size_t) x)*C,out);
}

// Row pitch of the staged planes: a 32-lane half of a wave reads 16 columns of two consecutive tile
// rows, so a pitch of 16 (mod 32) elements puts the two rows on disjoint LDS banks for 4- and
// 8-byte planes (2-byte planes share at most one bank).  The padding is dropped when only the
// plain pitch fits the budget.
static bool edge_layout(size_t W,size_t H,size_t fixed_bytes,size_t pixel_bytes,EdgeArgs *a,size_t *lds)
{
  const size_t tile_w=W+kEdgeBlock-1,tile_h=H+kEdgeBlock-1;
  size_t pitch=tile_w+((48u-(tile_w & 31u)) & 31u);
  if (fixed_bytes+pitch*tile_h*pixel_bytes > kEdgeMaxLds)
    pitch=(tile_w+3u) & ~(size_t) 3u;
  const size_t bytes=fixed_bytes+pitch*tile_h*pixel_bytes;
  if (bytes > kEdgeMaxLds)
    return false;
  a->width=(int) W;
  a->height=(int) H;
  a->tile_w=(int) tile_w;
  a->tile_h=(int) tile_h;
  a->pitch=(int) pitch;
  *lds=(bytes+15u) & ~(size_t) 15u;
  return true;
}

static MhStatus edge_frame(const View &src,const View &dst,const Roles &roles,const char *what,EdgeArgs *a)
{
  MH_TRY(window_grid_check(what,src));
  a->src=src.pixels;
  a->dst=dst.pixels;
  a->columns=(int) src.columns;
  a->rows=(int) src.rows;
  a->copy_mask=roles.copy_mask;
  a->alpha=roles.blend ? roles.alpha : -1;
  return MH_OK;
}

template<typename Q,int C,bool BILATERAL>
static MhStatus edge_launch(const EdgeArgs &a,size_t lds,hipStream_t stream)
{
  const dim3 grid=window_grid(a.columns,a.rows);
  if constexpr (BILATERAL)
    {
      MH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&bilateral_blur_kernel<Q,C>),
        hipFuncAttributeMaxDynamicSharedMemorySize,(int) kEdgeMaxLds));
      ProfileScope prof("bilateral_blur",stream);
      hipLaunchKernelGGL((bilateral_blur_kernel<Q,C>),grid,dim3(kEdgeBlock*kEdgeBlock),lds,stream,a);
    }
  else
    {
      MH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&selective_blur_kernel<Q,C>),
        hipFuncAttributeMaxDynamicSharedMemorySize,(int) kEdgeMaxLds));
      ProfileScope prof("selective_blur",stream);
      hipLaunchKernelGGL((selective_blur_kernel<Q,C>),grid,dim3(kEdgeBlock*kEdgeBlock),lds,stream,a);
    }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

template<bool BILATERAL>
static MhStatus edge_dispatch(const View &src,const EdgeArgs &a,size_t lds)
{
  return dispatch_layout(src.quantum,src.channels,[&](auto L) {
    return edge_launch<typename decltype(L)::Q,L.C,BILATERAL>(a,lds,src.stream); });
}

MhStatus launch_bilateral_blur(const View &src,const View &dst,size_t width,size_t height,
  double intensity_sigma,double spatial_sigma,const Roles &roles,const MhImage *desc)
{
  const size_t W=std::max<size_t>(width,1),H=std::max<size_t>(height,1);
  if (((W & 1u) == 0) || ((H & 1u) == 0))
    return fail(MH_UNSUPPORTED,"BilateralBlurImage: the reference reads outside its %zux%zu window when a "
      "side is even",W,H);
  if ((W > 4096) || (H > 4096))
    return fail(MH_UNSUPPORTED,"BilateralBlurImage: a %zux%zu window does not fit the LDS tile",W,H);
  if ((src.channels < 1) || (src.channels > 4))
    return fail(MH_UNSUPPORTED,"BilateralBlurImage: %d channels",src.channels);
  EdgeArgs a={};
  MH_TRY(edge_frame(src,dst,roles,"BilateralBlurImage",&a));
  // a staged pixel: its samples and one intensity byte; in front, the intensity Gaussian
  const size_t sample=src.quantum == MH_QUANTUM_U16 ? 2u : 4u;
  size_t lds=0;
  if (!edge_layout(W,H,kIntensityTable*sizeof(double),(size_t) src.channels*sample+1u,&a,&lds) ||
      (lds > (size_t) lds_bytes_per_workgroup(src.device)))
    return fail(MH_UNSUPPORTED,"BilateralBlurImage: a %zux%zu window does not fit the LDS tile",W,H);
  if ((src.columns == 0) || (src.rows == 0))
    return MH_OK;
  a.ip=intensity_params(desc);
  std::vector<double> tables(kIntensityTable+W*H);
  bilateral_blur_tables(W,H,intensity_sigma,spatial_sigma,tables.data(),tables.data()+kIntensityTable);
  Temp device_tables;
  MH_TRY(upload_table(device_tables,src.device,src.stream,tables.data(),tables.size()*sizeof(double)));
  a.tables=device_tables.as<double>();
  return edge_dispatch<true>(src,a,lds);
}

MhStatus launch_selective_blur(const View &src,const View &dst,double radius,double sigma,double threshold,
  const Roles &roles,const MhImage *desc)
{
  const size_t width=MhGetOptimalKernelWidth1D(radius,sigma);
  if (width > 4096)
    return fail(MH_UNSUPPORTED,"SelectiveBlurImage: a %zux%zu window does not fit the LDS tile",width,width);
  if ((src.channels < 1) || (src.channels > 4))
    return fail(MH_UNSUPPORTED,"SelectiveBlurImage: %d channels",src.channels);
  EdgeArgs a={};
  MH_TRY(edge_frame(src,dst,roles,"SelectiveBlurImage",&a));
  // the gray clone (effect.c:3510-3517): a gray image is left as it is; sRGB is weighed into one
  // Quantum; linear RGB goes through sRGB first.  The clone has one channel, two with alpha.
  const int colours=src.channels-(desc->alpha_offset >= 0 ? 1 : 0);
  const MhColorspace colorspace=(MhColorspace) desc->colorspace;
  if ((colours == 1) && ((colorspace == MH_COLORSPACE_SRGB) || (colorspace == MH_COLORSPACE_GRAY)))
    a.luminance=LUM_SELF;
  else if ((colours == 3) && (colorspace == MH_COLORSPACE_SRGB))
    a.luminance=LUM_FROM_SRGB;
  else if ((colours == 3) && (colorspace == MH_COLORSPACE_RGB))
    a.luminance=LUM_FROM_LINEAR;
  else
    return fail(MH_UNSUPPORTED,"SelectiveBlurImage: %d colour channels in colourspace %d",colours,
      (int) colorspace);
  if ((desc->alpha_offset >= 0) && (desc->alpha_offset != src.channels-1))
    return fail(MH_UNSUPPORTED,"SelectiveBlurImage: alpha is not the last channel");
  a.luminance_channels=src.channels-colours+1;
  a.ip=intensity_params(desc);
  a.luminance_ip=a.ip;
  a.luminance_ip.linear=0;
  a.luminance_ip.nonlinear=1;
  a.luminance_ip.gray=1;
  a.threshold=threshold;
  // blend channels compare the tap's own intensity, every other computed channel the clone's
  uint32_t plain=roles.update_mask;
  if (a.alpha >= 0)
    plain&=1u << a.alpha;
  a.stage_intensity=a.alpha >= 0 ? 1 : 0;
  a.stage_luminance=plain != 0 ? 1 : 0;
  // a staged pixel: its samples and the fp64 intensities the two comparisons need
  const size_t sample=src.quantum == MH_QUANTUM_U16 ? 2u : 4u;
  size_t lds=0;
  if (!edge_layout(width,width,0,(size_t) src.channels*sample+8u*(size_t) (a.stage_intensity+a.stage_luminance),
        &a,&lds) || (lds > (size_t) lds_bytes_per_workgroup(src.device)))
    return fail(MH_UNSUPPORTED,"SelectiveBlurImage: a %zux%zu window does not fit the LDS tile",width,width);
  if ((src.columns == 0) || (src.rows == 0))
    return MH_OK;
  std::vector<double> kernel(width*width);
  selective_blur_kernel_values(width,sigma,kernel.data());
  Temp device_kernel;
  MH_TRY(upload_table(device_kernel,src.device,src.stream,kernel.data(),kernel.size()*sizeof(double)));
  a.tables=device_kernel.as<double>();
  return edge_dispatch<false>(src,a,lds);
}

} // namespace mh
