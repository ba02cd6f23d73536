// Pointwise kernels of no larger family: CompositeImage, ContrastImage / ModulateImage (HSB, HSL), GrayscaleImage,
// FunctionImage, the gray scan, the unsharp-mask epilogue, and the layout helpers of operators.cpp and
// morphology_flat.hip: premultiply / separable finish, gray row bands, RGB pad / unpad and a plain copy.
//
// All of these stream every pixel once (HBM-bound): lanes take consecutive
// pixels with the widest load the pixel size allows, grid-stride over the
// image, >= 2048 workgroups.
//
// Reference semantics restated from:
//   GetPixelIntensity                      MagickCore/pixel.c:2356-2455
//   IdentifyImageGray                      MagickCore/attribute.c:1564-1626
//   UnsharpMaskImage epilogue              MagickCore/effect.c:4343-4372
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "pixel_intensity.hpp"
#include "colour_math.hpp"

namespace mh {

// ---------------------------------------------------------------- CompositeImage
// The two mathematical compositions MorphologyApply uses as post-steps (morphology.c:
// 3986-4044): Difference (EdgeIn/EdgeOut/Edge/TopHat/BottomHat) and Lighten (union of the
// HitAndMiss results of a kernel list).  Canvas and source have the same geometry, offset
// 0,0, default artifacts (compose:sync and compose:clamp on): composite.c:2396-2428 (alpha),
// :2523-2711 (alpha channel), :2716-2751 (Sca/Dca/gamma), :2922-2933 (Difference),
// :3110-3124 (Lighten), ClampPixel pixel-accessor.h:35-46.
enum CompositeKind { COMPOSITE_DIFFERENCE=0,COMPOSITE_LIGHTEN=1,COMPOSITE_DARKEN=2,COMPOSITE_PLUS=3,COMPOSITE_MULTIPLY=4,
  COMPOSITE_SCREEN=5,COMPOSITE_EXCLUSION=6,COMPOSITE_MINUS_SRC=7,COMPOSITE_MINUS_DST=8,COMPOSITE_LINEAR_DODGE=9,
  COMPOSITE_OVER=10,COMPOSITE_DST_OVER=11 };

template<typename Q> static __device__ __forceinline__ Q clamp_pixel(double pixel);
template<> __device__ __forceinline__ uint16_t clamp_pixel<uint16_t>(double pixel)
{
  if (pixel < 0.0)
    return 0;
  if (pixel >= kQR)
    return 65535;
  return (uint16_t) (pixel+0.5);
}
template<> __device__ __forceinline__ float clamp_pixel<float>(double pixel)
{
  if (pixel < 0.0)
    return 0.0f;
  if (pixel >= kQR)
    return 65535.0f;
  return (float) pixel;
}

template<typename Q,int C,int OP>
__global__ __launch_bounds__(256)
void composite_kernel(Q *__restrict__ canvas,const Q *__restrict__ source,size_t npixels,int alpha_index,
  uint32_t update_mask,uint32_t copy_mask)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      Q s[C],d[C];
      load_pixel<Q,C>(source+i*C,s);
      load_pixel<Q,C>(canvas+i*C,d);
      // GetPixelAlpha gives OpaqueAlpha for an image without an alpha channel
      const double Sa=kQS*(alpha_index >= 0 ? (double) s[alpha_index < 0 ? 0 : alpha_index] : kQR);
      const double Da=kQS*(alpha_index >= 0 ? (double) d[alpha_index < 0 ? 0 : alpha_index] : kQR);
      // Plus: RoundToUnity(source_dissolve*Sa+canvas_dissolve*Da), both 1 (composite.c:2462-2467);
      // the others RoundToUnity(Sa+Da-Sa*Da) (:2398-2426)
      double alpha=OP == COMPOSITE_PLUS ? 1.0*Sa+1.0*Da : Sa+Da-Sa*Da;
      if ((OP != COMPOSITE_OVER) && (OP != COMPOSITE_DST_OVER))      // (Over / DstOver: not rounded to unity, :2443-2449)
        alpha=alpha < 0.0 ? 0.0 : (alpha > 1.0 ? 1.0 : alpha);
      // composite.c:2737-2751
      const double gamma=perceptible_reciprocal(((OP == COMPOSITE_LIGHTEN) || (OP == COMPOSITE_DARKEN)) ? 1.0-alpha : alpha);
#pragma unroll
      for (int c=0; c < C; c++)
        {
          // CompositeOverImage sets the alpha channel whatever its trait says, Update or Copy
          // (composite.c:1096-1104): `-channel RGB` does not keep the merged alpha out
          if ((c == alpha_index) && ((OP == COMPOSITE_OVER) || (((update_mask >> c) & 1u) != 0)))
            {
              // composite.c:2580-2712 (Multiply with synchronised channels: the default case)
              const double pixel=OP == COMPOSITE_DIFFERENCE ? kQR*fabs(Sa-Da) : kQR*alpha;
              d[c]=clamp_pixel<Q>(pixel);
              continue;
            }
          if (((copy_mask >> c) & 1u) != 0)
            {
              // ClampToQuantum(Dc) = Dc; Over runs CompositeOverImage (composite.c:1489-1495), whose
              // copy channels take the SOURCE (:1115-1121)
              if (OP == COMPOSITE_OVER)
                d[c]=s[c];
              continue;
            }
          const double Sc=(double) s[c],Dc=(double) d[c];
          const double Sca=kQS*Sa*Sc,Dca=kQS*Da*Dc;
          double pixel;
          if (OP == COMPOSITE_DIFFERENCE)
            {
              const double a=Sca*Da,b=Dca*Sa;
              pixel=kQR*gamma*(Sca+Dca-2.0*(a < b ? a : b));
            }
          else if (OP == COMPOSITE_PLUS)
            pixel=kQR*(Sca+Dca);                                 // composite.c:3369-3378
          else if (OP == COMPOSITE_MULTIPLY)
            pixel=kQR*gamma*(Sca*Dca+Sca*(1.0-Da)+Dca*(1.0-Sa)); // :3288-3299
          else if (OP == COMPOSITE_SCREEN)
            pixel=kQR*gamma*(Sca+Dca-Sca*Dca);                   // :3447-3461
          else if (OP == COMPOSITE_EXCLUSION)
            pixel=kQR*gamma*(Sca*Da+Dca*Sa-2.0*Sca*Dca+Sca*(1.0-Da)+Dca*(1.0-Sa));   // :3011-3016
          else if (OP == COMPOSITE_MINUS_SRC)
            pixel=gamma*(Da*Dc+Sa*Sc-2.0*Sa*Sc*Da);              // :3211-3224
          else if (OP == COMPOSITE_MINUS_DST)
            pixel=gamma*(Sa*Sc+Da*Dc-2.0*Da*Dc*Sa);              // :3201-3210
          else if (OP == COMPOSITE_LINEAR_DODGE)
            pixel=gamma*(Sa*Sc+Da*Dc);                           // :3094-3098
          else if (OP == COMPOSITE_OVER)
            pixel=kQR*gamma*(Sca+Dca*(1.0-Sa));                  // :3310-3315
          else if (OP == COMPOSITE_DST_OVER)
            pixel=kQR*gamma*(Dca+Sca*(1.0-Da));                  // :3006-3010
          else if (OP == COMPOSITE_DARKEN ? (Sca*Da) < (Dca*Sa) : (Sca*Da) > (Dca*Sa))
            pixel=kQR*(Sca+Dca*(1.0-Sa));                        // :2892-2910, :3110-3124
          else
            pixel=kQR*(Dca+Sca*(1.0-Da));
          d[c]=clamp_pixel<Q>(pixel);
        }
      store_pixel<Q,C>(canvas+i*C,d);
    }
}

template<typename Q,int C>
static MhStatus composite_typed(const View &canvas,const View &source,int kind,const Roles &roles)
{
  const size_t n=canvas.columns*canvas.rows;
  dim3 grid(stream_grid(n)),block(256);
  ProfileScope prof("composite",canvas.stream);
#define MH_COMPOSE(OP) \
  hipLaunchKernelGGL((composite_kernel<Q,C,OP>),grid,block,0,canvas.stream,static_cast<Q *>(canvas.pixels), \
    static_cast<const Q *>(source.pixels),n,roles.alpha,roles.update_mask,roles.copy_mask)
  switch (kind)
  {
    case COMPOSITE_DIFFERENCE: MH_COMPOSE(COMPOSITE_DIFFERENCE); break;
    case COMPOSITE_LIGHTEN: MH_COMPOSE(COMPOSITE_LIGHTEN); break;
    case COMPOSITE_DARKEN: MH_COMPOSE(COMPOSITE_DARKEN); break;
    case COMPOSITE_PLUS: MH_COMPOSE(COMPOSITE_PLUS); break;
    case COMPOSITE_MULTIPLY: MH_COMPOSE(COMPOSITE_MULTIPLY); break;
    case COMPOSITE_SCREEN: MH_COMPOSE(COMPOSITE_SCREEN); break;
    case COMPOSITE_EXCLUSION: MH_COMPOSE(COMPOSITE_EXCLUSION); break;
    case COMPOSITE_MINUS_SRC: MH_COMPOSE(COMPOSITE_MINUS_SRC); break;
    case COMPOSITE_MINUS_DST: MH_COMPOSE(COMPOSITE_MINUS_DST); break;
    case COMPOSITE_LINEAR_DODGE: MH_COMPOSE(COMPOSITE_LINEAR_DODGE); break;
    case COMPOSITE_OVER: MH_COMPOSE(COMPOSITE_OVER); break;
    case COMPOSITE_DST_OVER: MH_COMPOSE(COMPOSITE_DST_OVER); break;
    default: return fail(MH_UNSUPPORTED,"composite operator %d",kind);
  }
#undef MH_COMPOSE
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_composite(const View &canvas,const View &source,int kind,const Roles &roles)
{
  if ((canvas.columns != source.columns) || (canvas.rows != source.rows) ||
      (canvas.channels != source.channels) || (canvas.quantum != source.quantum))
    return fail(MH_BAD_ARGUMENT,"composite: canvas and source differ in geometry");
  return dispatch_layout(canvas.quantum,canvas.channels,[&](auto L) {
    return composite_typed<typename decltype(L)::Q,L.C>(canvas,source,kind,roles); });
}

// ---------------------------------------------------------------- ContrastImage / ModulateImage
// (the HSB and HSL round trips: colour_math.hpp)
enum ToneOp { TONE_CONTRAST=0,TONE_MODULATE_HSL=1,TONE_MODULATE_HSB=2 };

struct ToneArgs
{
  int op;
  double sign;                 // Contrast: +1 sharpen, -1 dull
  double hue_shift,saturation_scale,brightness_scale;      // Modulate
};

// ContrastImage enhance.c:1370-1390 (per pixel), ModulateHSL / ModulateHSB :3499-3554
template<typename Q,int C>
__global__ __launch_bounds__(256)
void tone_kernel(Q *__restrict__ pixels,size_t npixels,ToneArgs a)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x*kPointBatch;
  for (size_t i0=(size_t) blockIdx.x*blockDim.x*kPointBatch+threadIdx.x; i0 < npixels; i0+=stride)
    {
      Q qb[kPointBatch][C];
#pragma unroll
      for (int k=0; k < kPointBatch; k++)
        {
          const size_t ik=i0+(size_t) k*blockDim.x;
          load_pixel<Q,C>(pixels+(ik < npixels ? ik : npixels-1)*C,qb[k]);
        }
#pragma unroll
      for (int k=0; k < kPointBatch; k++)
        {
          const size_t i=i0+(size_t) k*blockDim.x;
          double red=(double) qb[k][0],green=(double) qb[k][1],blue=(double) qb[k][2];
          double hue,saturation,third;
          if (a.op == TONE_CONTRAST)
            {
              rgb_to_hsb(red,green,blue,hue,saturation,third);
              third+=0.5*a.sign*(0.5*(sin((double) (3.14159265358979323846264338327950288*(third-0.5)))+1.0)-third);
              third=third > 1.0 ? 1.0 : (third < 0.0 ? 0.0 : third);
              hsb_to_rgb(hue,saturation,third,red,green,blue);
            }
          else if (a.op == TONE_MODULATE_HSB)
            {
              rgb_to_hsb(red,green,blue,hue,saturation,third);
              hue+=a.hue_shift;
              saturation*=a.saturation_scale;
              third*=a.brightness_scale;
              hsb_to_rgb(hue,saturation,third,red,green,blue);
            }
          else
            {
              rgb_to_hsl(red,green,blue,hue,saturation,third);
              hue+=a.hue_shift;
              saturation*=a.saturation_scale;
              third*=a.brightness_scale;
              hsl_to_rgb(hue,saturation,third,red,green,blue);
            }
          qb[k][0]=QuantumOps<Q>::clamp(red);
          qb[k][1]=QuantumOps<Q>::clamp(green);
          qb[k][2]=QuantumOps<Q>::clamp(blue);
          if (i < npixels)
            store_pixel<Q,C>(pixels+i*C,qb[k]);
        }
    }
}

static MhStatus launch_tone(const View &img,const ToneArgs &a,const char *label)
{
  if ((img.channels != 3) && (img.channels != 4))
    return fail(MH_UNSUPPORTED,"%s needs R,G,B[,A] channels",label);
  const size_t n=img.columns*img.rows;
  dim3 grid(stream_grid((n+kPointBatch-1)/kPointBatch)),block(256);
  ProfileScope prof(label,img.stream);
  dispatch_colour_layout(img.quantum,img.channels,[&](auto L) {
    using Q=typename decltype(L)::Q;
    hipLaunchKernelGGL((tone_kernel<Q,L.C>),grid,block,0,img.stream,static_cast<Q *>(img.pixels),n,a); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_contrast(const View &img,bool sharpen)
{
  ToneArgs a;
  a.op=TONE_CONTRAST;
  a.sign=sharpen ? 1.0 : -1.0;
  a.hue_shift=a.saturation_scale=a.brightness_scale=0.0;
  return launch_tone(img,a,"contrast");
}

MhStatus launch_modulate(const View &img,bool hsb,double hue_shift,double saturation_scale,
  double brightness_scale)
{
  ToneArgs a;
  a.op=hsb ? TONE_MODULATE_HSB : TONE_MODULATE_HSL;
  a.sign=0.0;
  a.hue_shift=hue_shift;
  a.saturation_scale=saturation_scale;
  a.brightness_scale=brightness_scale;
  return launch_tone(img,a,"modulate");
}

// ---------------------------------------------------------------- GrayscaleImage
// enhance.c:2476-2660: the intensity of (R,G,B) by `method` is written to the Gray
// (= first) channel only; the caller then switches the image to GRAY / LinearGRAY.
// Note MS here is (r^2+g^2+b^2)/3 (:2572-2577), unlike GetPixelIntensity's MS.
template<typename Q,int C>
__global__ __launch_bounds__(256)
void grayscale_kernel(Q *pixels,size_t npixels,int method,int is_rgb,int is_srgb)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+i*C,q);
      double red=(double) q[0],green=(double) q[C >= 3 ? 1 : 0],blue=(double) q[C >= 3 ? 2 : 0];
      double intensity=0.0;
      switch (method)
      {
        case MH_INTENSITY_AVERAGE: intensity=(red+green+blue)/3.0; break;
        case MH_INTENSITY_BRIGHTNESS:
        {
          double m=red > green ? red : green;
          intensity=m > blue ? m : blue;
          break;
        }
        case MH_INTENSITY_LIGHTNESS:
        {
          double mn=red < green ? red : green;
          mn=mn < blue ? mn : blue;
          double mx=red > green ? red : green;
          mx=mx > blue ? mx : blue;
          intensity=(mn+mx)/2.0;
          break;
        }
        case MH_INTENSITY_MS: intensity=(red*red+green*green+blue*blue)/3.0; break;
        case MH_INTENSITY_RMS: intensity=sqrt(red*red+green*green+blue*blue)/sqrt(3.0); break;
        case MH_INTENSITY_REC601LUMA:
        case MH_INTENSITY_REC601LUMINANCE:
        {
          if ((method == MH_INTENSITY_REC601LUMA) ? is_rgb : is_srgb)
            {
              if (method == MH_INTENSITY_REC601LUMA)
                { red=encode_pixel_gamma(red); green=encode_pixel_gamma(green); blue=encode_pixel_gamma(blue); }
              else
                { red=decode_pixel_gamma(red); green=decode_pixel_gamma(green); blue=decode_pixel_gamma(blue); }
            }
          intensity=0.298839*red+0.586811*green+0.114350*blue;
          break;
        }
        case MH_INTENSITY_REC709LUMINANCE:
        {
          if (is_srgb)
            { red=decode_pixel_gamma(red); green=decode_pixel_gamma(green); blue=decode_pixel_gamma(blue); }
          intensity=0.212656*red+0.715158*green+0.072186*blue;
          break;
        }
        default:      // Rec709Luma
        {
          if (is_rgb)
            { red=encode_pixel_gamma(red); green=encode_pixel_gamma(green); blue=encode_pixel_gamma(blue); }
          intensity=0.212656*red+0.715158*green+0.072186*blue;
          break;
        }
      }
      pixels[i*C]=QuantumOps<Q>::clamp(intensity);       // SetPixelGray: the first channel only
    }
}

MhStatus launch_grayscale(const View &img,int method,const MhImage *desc)
{
  const size_t n=img.columns*img.rows;
  const int is_rgb=desc->colorspace == MH_COLORSPACE_RGB;
  const int is_srgb=desc->colorspace == MH_COLORSPACE_SRGB;
  ProfileScope prof("grayscale",img.stream);
  dispatch_layout(img.quantum,img.channels,[&](auto L) {
    using Q=typename decltype(L)::Q;
    hipLaunchKernelGGL((grayscale_kernel<Q,L.C>),dim3(stream_grid(n)),dim3(256),0,img.stream,
      static_cast<Q *>(img.pixels),n,method,is_rgb,is_srgb); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ----------------------------------------------------------------- FunctionImage
// ApplyFunction, statistic.c:975-1067, on every channel selected by `mask`.
struct FunctionParams
{
  int function;               // MhFunction
  int count;
  double p[8];
};

template<typename Q,int C>
__global__ __launch_bounds__(256)
void function_kernel(Q *pixels,size_t npixels,FunctionParams fp,uint32_t mask)
{
  // (kPi: MagickPI, colour_math.hpp)
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+i*C,q);
#pragma unroll
      for (int c=0; c < C; c++)
        {
          if (((mask >> c) & 1u) == 0)
            continue;
          const double pixel=(double) q[c];
          double result=0.0;
          switch (fp.function)
          {
            case MH_FUNCTION_POLYNOMIAL:
              for (int k=0; k < fp.count; k++)
                result=result*kQS*pixel+fp.p[k];
              result*=kQR;
              break;
            case MH_FUNCTION_SINUSOID:
            {
              double frequency=fp.count >= 1 ? fp.p[0] : 1.0,phase=fp.count >= 2 ? fp.p[1] : 0.0;
              double amplitude=fp.count >= 3 ? fp.p[2] : 0.5,bias=fp.count >= 4 ? fp.p[3] : 0.5;
              result=kQR*(amplitude*sin(2.0*kPi*(frequency*kQS*pixel+phase/360.0))+bias);
              break;
            }
            case MH_FUNCTION_ARCSIN:
            {
              double width=fp.count >= 1 ? fp.p[0] : 1.0,center=fp.count >= 2 ? fp.p[1] : 0.5;
              double range=fp.count >= 3 ? fp.p[2] : 1.0,bias=fp.count >= 4 ? fp.p[3] : 0.5;
              result=2.0*perceptible_reciprocal(width)*(kQS*pixel-center);
              if (result <= -1.0)
                result=bias-range/2.0;
              else if (result >= 1.0)
                result=bias+range/2.0;
              else
                result=range/kPi*asin(result)+bias;
              result*=kQR;
              break;
            }
            case MH_FUNCTION_ARCTAN:
            {
              double slope=fp.count >= 1 ? fp.p[0] : 1.0,center=fp.count >= 2 ? fp.p[1] : 0.5;
              double range=fp.count >= 3 ? fp.p[2] : 1.0,bias=fp.count >= 4 ? fp.p[3] : 0.5;
              result=kPi*slope*(kQS*pixel-center);
              result=kQR*(range/kPi*atan(result)+bias);
              break;
            }
            default: break;
          }
          q[c]=QuantumOps<Q>::clamp(result);
        }
      store_pixel<Q,C>(pixels+i*C,q);
    }
}

MhStatus launch_function(const View &img,int function,size_t count,const double *parameters,uint32_t mask)
{
  if (count > 8)
    return fail(MH_UNSUPPORTED,"FunctionImage: more than 8 parameters");
  FunctionParams fp;
  fp.function=function;
  fp.count=(int) count;
  for (int k=0; k < 8; k++)
    fp.p[k]=k < (int) count ? parameters[k] : 0.0;
  const size_t n=img.columns*img.rows;
  ProfileScope prof("function",img.stream);
  dispatch_layout(img.quantum,img.channels,[&](auto L) {
    using Q=typename decltype(L)::Q;
    hipLaunchKernelGGL((function_kernel<Q,L.C>),dim3(stream_grid(n)),dim3(256),0,img.stream,
      static_cast<Q *>(img.pixels),n,fp,mask); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ---------------------------------------------------------------- gray scan
// SetImageGray's scan (attribute.c:1416-1450: IsPixelGray on every pixel).  A wave leaves at its
// first colour pixel and reports it with a plain store — on a colour frame the kernel used to be
// 32 768 atomicOr on one word (0.4 ms per 8192^2 RGBA call, more than the histogram) — and Q16
// pixels are compared as integers (|a-b| <
// MagickEpsilon on integer levels is a == b), two RGBA pixels per 16-byte load.
template<typename Q,int C>
__global__ __launch_bounds__(256)
void gray_check_kernel(const Q *pixels,size_t npixels,unsigned int *not_gray)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  bool bad=false;
  if constexpr ((sizeof(Q) == 2) && (C == 4))
    {
      if ((reinterpret_cast<uintptr_t>(pixels) & 15u) == 0)
        {
          const uint4 *pairs=reinterpret_cast<const uint4 *>(pixels);
          const size_t npairs=npixels/2;
          for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npairs; i+=stride)
            {
              const uint4 v=pairs[i];
              // red == green and green == blue, both pixels
              bad=(((v.x >> 16) ^ v.x) & 0xffffu) != 0u || ((v.y ^ v.x) & 0xffffu) != 0u ||
                  (((v.z >> 16) ^ v.z) & 0xffffu) != 0u || ((v.w ^ v.z) & 0xffffu) != 0u;
              if (__any(bad))
                break;
            }
          if (((npixels & 1u) != 0) && (blockIdx.x == 0) && (threadIdx.x == 0))
            {
              const uint16_t *last=pixels+(npixels-1)*4;
              bad=bad || (last[0] != last[1]) || (last[1] != last[2]);
            }
          if (__any(bad) && ((threadIdx.x & 63) == 0))
            *not_gray=1u;                        // (a plain store: every writer writes the same 1)
          return;
        }
    }
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+i*C,q);
      // IsPixelGray, pixel-accessor.h: |red-green| < eps && |green-blue| < eps
      double rg=(double) q[0]-(double) q[1],gb=(double) q[1]-(double) q[2];
      if (!((fabs(rg) < kEps) && (fabs(gb) < kEps)))
        bad=true;
      if (__any(bad))
        break;
    }
  if (__any(bad) && ((threadIdx.x & 63) == 0))
    *not_gray=1u;
}

MhStatus launch_gray_check(const View &img,const MhImage *,unsigned int *flag)
{
  const size_t n=img.columns*img.rows;
  dim3 grid(stream_grid(n)),block(256);
  ProfileScope prof("gray_check",img.stream);
  dispatch_colour_layout(img.quantum,img.channels,[&](auto L) {
    using Q=typename decltype(L)::Q;
    hipLaunchKernelGGL((gray_check_kernel<Q,L.C>),grid,block,0,img.stream,
      static_cast<const Q *>(img.pixels),n,flag); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ------------------------------------------------------- unsharp epilogue
template<typename Q,int C>
__global__ __launch_bounds__(256)
void unsharp_kernel(const Q *src,const Q *blur,Q *dst,size_t npixels,double gain,
  double quantum_threshold,uint32_t copy_mask)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      Q p[C],b[C],o[C];
      load_pixel<Q,C>(src+i*C,p);
      load_pixel<Q,C>(blur+i*C,b);
#pragma unroll
      for (int c=0; c < C; c++)
        {
          if ((copy_mask >> c) & 1u)
            {
              o[c]=p[c];
              continue;
            }
          // effect.c:4364-4369
          double pixel=(double) p[c]-(double) b[c];
          if (fabs(2.0*pixel) < quantum_threshold)
            pixel=(double) p[c];
          else
            pixel=(double) p[c]+gain*pixel;
          o[c]=QuantumOps<Q>::clamp(pixel);
        }
      store_pixel<Q,C>(dst+i*C,o);
    }
}

template<typename Q,int C>
static MhStatus unsharp_typed(const View &src,const View &blur,const View &dst,double gain,
  double threshold,uint32_t copy_mask)
{
  const size_t n=src.columns*src.rows;
  ProfileScope prof("unsharp_epilogue",src.stream);
  hipLaunchKernelGGL((unsharp_kernel<Q,C>),dim3(stream_grid(n)),dim3(256),0,src.stream,
    static_cast<const Q *>(src.pixels),static_cast<const Q *>(blur.pixels),
    static_cast<Q *>(dst.pixels),n,gain,kQuantumRange*threshold,copy_mask);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_unsharp_epilogue(const View &src,const View &blur,const View &dst,double gain,
  double threshold,const Roles &roles)
{
  return dispatch_layout(src.quantum,src.channels,[&](auto L) {
    return unsharp_typed<typename decltype(L)::Q,L.C>(src,blur,dst,gain,threshold,roles.copy_mask); });
}

// ------------------------------------------- separable 2-D convolution, FAST
// A rank-1 2-D kernel (Gaussian:RxS ...) is run as a row and a column pass over float sums.
// The reference's 2-D loop (morphology.c:2892-2979) forms sum k*alpha*p and sum k*alpha over
// the whole window and divides once, so the passes must carry the *undivided* sums:
// premultiply_kernel writes alpha*p (alpha = QuantumScale*a) and a as floats, the two 1-D
// passes convolve those as plain channels, separable_finish_kernel divides and quantises.
template<int C,bool BLEND>
__global__ __launch_bounds__(256)
void premultiply_kernel(const uint16_t *src,float *dst,size_t npixels)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      uint16_t p[C];
      float o[C];
      load_pixel<uint16_t,C>(src+i*C,p);
      const float alpha=BLEND ? (float) p[C-1]*(1.0f/65535.0f) : 1.0f;
#pragma unroll
      for (int c=0; c < C; c++)
        o[c]=BLEND && (c < C-1) ? alpha*(float) p[c] : (float) p[c];
      store_pixel<float,C>(dst+i*C,o);
    }
}

template<int C,bool BLEND>
__global__ __launch_bounds__(256)
void separable_finish_kernel(const float *sums,uint16_t *dst,size_t npixels)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      float v[C];
      uint16_t o[C];
      load_pixel<float,C>(sums+i*C,v);
      // gamma = 1/sum(k*alpha) = 65535/v[alpha]; an all-transparent window has zero sums: 0
      const float gamma=BLEND ? (v[C-1] > 0.0f ? 65535.0f/v[C-1] : 0.0f) : 1.0f;
#pragma unroll
      for (int c=0; c < C; c++)
        {
          const float pixel=BLEND && (c < C-1) ? gamma*v[c] : v[c];
          const float q=floorf(pixel+0.5f);
          o[c]=(uint16_t) (q < 0.0f ? 0.0f : (q > 65535.0f ? 65535.0f : q));
        }
      store_pixel<uint16_t,C>(dst+i*C,o);
    }
}

MhStatus launch_premultiply(const View &src,const View &sums,bool blend)
{
  if ((src.channels < 1) || (src.channels > 4))
    return fail(MH_UNSUPPORTED,"separable convolution: %d channels",src.channels);
  const size_t n=src.columns*src.rows;
  const uint16_t *in=static_cast<const uint16_t *>(src.pixels);
  float *out=static_cast<float *>(sums.pixels);
  ProfileScope prof("premultiply",src.stream);
  dispatch_layout_blend(src.quantum,src.channels,blend,[&](auto L) {
    hipLaunchKernelGGL((premultiply_kernel<L.C,L.BLEND>),dim3(stream_grid(n)),dim3(256),0,src.stream,in,out,n); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_separable_finish(const View &sums,const View &dst,bool blend)
{
  if ((dst.channels < 1) || (dst.channels > 4))
    return fail(MH_UNSUPPORTED,"separable convolution: %d channels",dst.channels);
  const size_t n=dst.columns*dst.rows;
  const float *in=static_cast<const float *>(sums.pixels);
  uint16_t *out=static_cast<uint16_t *>(dst.pixels);
  ProfileScope prof("separable_finish",dst.stream);
  dispatch_layout_blend(dst.quantum,dst.channels,blend,[&](auto L) {
    hipLaunchKernelGGL((separable_finish_kernel<L.C,L.BLEND>),dim3(stream_grid(n)),dim3(256),0,dst.stream,in,out,n); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ------------------------------------------------------------------ one-channel frames as four row bands
// A gray Q16 frame has no wide pixel to hand the one-launch blur kernels (convolve_fused_hybrid.hip,
// convolve_fused_exact.hip: 8-byte pixels, four independent channels).  Its rows cut into four bands ARE four
// independent channels of a frame a quarter as tall: channel c of packed row r is source row c*band + r - halo,
// clamped into the frame (the virtual pixels of cache.c:2663-2679 above the first and below the last row; between
// bands, the neighbouring band's real rows).  The kernels' own edge clamp then only ever decides packed rows
// [0, halo) and [band+halo, band+2*halo), which unpacking drops.
__global__ __launch_bounds__(256)
void gray_bands_pack_kernel(const uint16_t *src,uint16_t *dst,int W,int H,int band,int halo)
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x);
  const int r=(int) blockIdx.y;
  if (x >= W)
    return;
  uint16_t p[4];
#pragma unroll
  for (int c=0; c < 4; c++)
    {
      int y=c*band+r-halo;
      y=y < 0 ? 0 : (y > H-1 ? H-1 : y);
      p[c]=src[(size_t) y*(size_t) W+(size_t) x];
    }
  store_pixel<uint16_t,4>(dst+((size_t) r*(size_t) W+(size_t) x)*4,p);
}

// ... and back; `changed` (MorphologyPrimitive's count, morphology.c:3199): the samples that differ from `original`
__global__ __launch_bounds__(256)
void gray_bands_unpack_kernel(const uint16_t *src,uint16_t *dst,int W,int H,int band,int halo,
  const uint16_t *original,unsigned long long *changed)
{
  const int x=(int) (blockIdx.x*blockDim.x+threadIdx.x);
  const int r=(int) blockIdx.y;
  unsigned differ=0;
  if (x < W)
    {
      uint16_t p[4];
      load_pixel<uint16_t,4>(src+((size_t) (r+halo)*(size_t) W+(size_t) x)*4,p);
#pragma unroll
      for (int c=0; c < 4; c++)
        {
          const int y=c*band+r;
          if (y < H)
            {
              const size_t at=(size_t) y*(size_t) W+(size_t) x;
              if (changed != nullptr)
                differ+=original[at] != p[c] ? 1u : 0u;
              dst[at]=p[c];
            }
        }
    }
  if (changed != nullptr)
    {
      differ=wave_sum(differ);
      if (((threadIdx.x & 63) == 0) && (differ != 0))
        atomicAdd(changed,(unsigned long long) differ);
    }
}

MhStatus launch_gray_bands_pack(const View &src,const View &packed,int band,int halo)
{
  ProfileScope prof("gray_bands_pack",src.stream);
  hipLaunchKernelGGL(gray_bands_pack_kernel,dim3((unsigned) ((src.columns+255)/256),(unsigned) (band+2*halo)),dim3(256),0,
    src.stream,static_cast<const uint16_t *>(src.pixels),static_cast<uint16_t *>(packed.pixels),(int) src.columns,
    (int) src.rows,band,halo);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_gray_bands_unpack(const View &packed,const View &dst,int band,int halo,const void *original,
  unsigned long long *changed)
{
  ProfileScope prof("gray_bands_unpack",dst.stream);
  hipLaunchKernelGGL(gray_bands_unpack_kernel,dim3((unsigned) ((dst.columns+255)/256),(unsigned) band),dim3(256),0,
    dst.stream,static_cast<const uint16_t *>(packed.pixels),static_cast<uint16_t *>(dst.pixels),(int) dst.columns,
    (int) dst.rows,band,halo,static_cast<const uint16_t *>(original),changed);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// ------------------------------------------------------------------ three-channel frames with a fourth, empty one
// RGB without alpha — 6-byte (Q16) or 12-byte (float) pixels — has no vector load of its own either; the
// union-of-rectangles kernel (morphology_flat.hip) takes 8- and 16-byte pixels.  Padded to four channels (the fourth 0) it
// is an ordinary four-channel frame; minima and maxima are per channel.
template<typename Q>
__global__ __launch_bounds__(256)
void rgb_pad_kernel(const Q *src,Q *dst,size_t npixels)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      Q p[3],o[4];
      load_pixel<Q,3>(src+i*3,p);
      o[0]=p[0]; o[1]=p[1]; o[2]=p[2]; o[3]=(Q) 0;
      store_pixel<Q,4>(dst+i*4,o);
    }
}

// ... and back; `changed` counts the samples with |result - original| >= MagickEpsilon (morphology.c:3195-3199; a
// NaN difference is not one)
template<typename Q>
__global__ __launch_bounds__(256)
void rgb_unpad_kernel(const Q *src,Q *dst,size_t npixels,const Q *original,unsigned long long *changed)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  unsigned differ=0;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < npixels; i+=stride)
    {
      Q p[4],o[3];
      load_pixel<Q,4>(src+i*4,p);
      o[0]=p[0]; o[1]=p[1]; o[2]=p[2];
      if (changed != nullptr)
        {
          Q was[3];
          load_pixel<Q,3>(original+i*3,was);
#pragma unroll
          for (int c=0; c < 3; c++)
            differ+=fabs((double) o[c]-(double) was[c]) >= 1.0e-12 ? 1u : 0u;
        }
      store_pixel<Q,3>(dst+i*3,o);
    }
  if (changed != nullptr)
    {
      differ=wave_sum(differ);
      if (((threadIdx.x & 63) == 0) && (differ != 0))
        atomicAdd(changed,(unsigned long long) differ);
    }
}

MhStatus launch_rgb_pad(const View &src,const View &padded)
{
  const size_t n=src.columns*src.rows;
  ProfileScope prof("rgb_pad",src.stream);
  if (src.quantum == MH_QUANTUM_U16)
    hipLaunchKernelGGL(rgb_pad_kernel<uint16_t>,dim3(stream_grid(n)),dim3(256),0,src.stream,
      static_cast<const uint16_t *>(src.pixels),static_cast<uint16_t *>(padded.pixels),n);
  else
    hipLaunchKernelGGL(rgb_pad_kernel<float>,dim3(stream_grid(n)),dim3(256),0,src.stream,
      static_cast<const float *>(src.pixels),static_cast<float *>(padded.pixels),n);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_rgb_unpad(const View &padded,const View &dst,const void *original,unsigned long long *changed)
{
  const size_t n=dst.columns*dst.rows;
  ProfileScope prof("rgb_unpad",dst.stream);
  if (dst.quantum == MH_QUANTUM_U16)
    hipLaunchKernelGGL((rgb_unpad_kernel<uint16_t>),dim3(stream_grid(n)),dim3(256),0,dst.stream,
      static_cast<const uint16_t *>(padded.pixels),static_cast<uint16_t *>(dst.pixels),n,
      static_cast<const uint16_t *>(original),changed);
  else
    hipLaunchKernelGGL((rgb_unpad_kernel<float>),dim3(stream_grid(n)),dim3(256),0,dst.stream,
      static_cast<const float *>(padded.pixels),static_cast<float *>(dst.pixels),n,
      static_cast<const float *>(original),changed);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

MhStatus launch_copy(const View &src,const View &dst)
{
  MH_HIP(hipMemcpyAsync(dst.pixels,src.pixels,src.bytes(),hipMemcpyDeviceToDevice,src.stream));
  return MH_OK;
}

} // namespace mh
