// Colourspace transforms: sRGB <-> linear RGB / Lab / XYZ in fp64, the per-device Q16 transfer tables, the two
// FAST f32 Lab kernels, the pointwise colourspaces of ConvertRGBToGeneric / ConvertGenericToRGB
// (colorspace_generic.hpp), the table-driven ones (OHTA, Rec601 / Rec709 YCbCr, YCC) and Log.
//
// All of these stream every pixel once (HBM-bound): lanes take consecutive
// pixels with the widest load the pixel size allows, grid-stride over the
// image, >= 2048 workgroups.
//
// Reference semantics restated from:
//   DecodePixelGamma / EncodePixelGamma   MagickCore/pixel.c:260-324, :380-451
//   ConvertRGBToXYZ / XYZToLab / LabToXYZ / XYZToRGB
//                                          MagickCore/colorspace-private.h:759-779, :1066-1089, :531-557, :72-94
//   sRGBTransformImage / TransformsRGBImage MagickCore/colorspace.c:1031-1049, :1203-1214, :2373-2381, :2541-2552
#include "mh_internal.hpp"
#include "device_common.hpp"
#include "layout_dispatch.hpp"
#include "pixel_intensity.hpp"
#include "colour_math.hpp"
#include "colorspace_generic.hpp"

#include <cmath>
#include <map>
#include <mutex>
#include <vector>

namespace mh {

enum ColorOp
{
  OP_SRGB_TO_RGB,OP_RGB_TO_SRGB,OP_SRGB_TO_LAB,OP_LAB_TO_SRGB,OP_SRGB_TO_XYZ,OP_XYZ_TO_SRGB
};

// Q16 pixels have only 65536 possible sRGB samples, so the transfer functions are tabulated
// once per device by the same device code that evaluates them per pixel (bit-identical):
// QuantumScale*DecodePixelGamma(j) as doubles (512 KB, L2-resident) for the XYZ/Lab kernels,
// and the Quantum-rounded decode / encode columns for sRGB <-> linear RGB, which then run as
// LUT applications.
__global__ __launch_bounds__(256)
void colorspace_table_kernel(double *decode_scaled,uint16_t *decode_q16,uint16_t *encode_q16)
{
  const unsigned j=blockIdx.x*blockDim.x+threadIdx.x;
  if (j > 65535u)
    return;
  const double d=decode_pixel_gamma((double) j);
  decode_scaled[j]=kQS*d;
  decode_q16[j]=QuantumOps<uint16_t>::clamp(d);
  encode_q16[j]=QuantumOps<uint16_t>::clamp(encode_pixel_gamma((double) j));
}

template<int C,int OP>
__global__ __launch_bounds__(256)
void colorspace_q16_table_kernel(uint16_t *__restrict__ pixels,size_t npixels,
  const double *__restrict__ decode_scaled)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x*kPointBatch;
  for (size_t i0=(size_t) blockIdx.x*blockDim.x*kPointBatch+threadIdx.x; i0 < npixels; i0+=stride)
    {
      uint16_t q[kPointBatch][C];
#pragma unroll
      for (int k=0; k < kPointBatch; k++)
        {
          const size_t i=i0+(size_t) k*blockDim.x;
          load_pixel<uint16_t,C>(pixels+(i < npixels ? i : npixels-1)*C,q[k]);
        }
      // ConvertRGBToXYZ, colorspace-private.h:759-779, with the three decodes looked up
      double r[kPointBatch],g[kPointBatch],b[kPointBatch];
#pragma unroll
      for (int k=0; k < kPointBatch; k++)
        {
          r[k]=decode_scaled[q[k][0]];
          g[k]=decode_scaled[q[k][1]];
          b[k]=decode_scaled[q[k][2]];
        }
#pragma unroll
      for (int k=0; k < kPointBatch; k++)
        {
          const double X=(0.4123955889674142161*r[k])+(0.3575834307637148171*g[k])+(0.1804926473817015735*b[k]);
          const double Y=(0.2125862307855955516*r[k])+(0.7151703037034108499*g[k])+(0.07220049864333622685*b[k]);
          const double Z=(0.01929721549174694484*r[k])+(0.1191838645808485318*g[k])+(0.9504971251315797660*b[k]);
          double o0,o1,o2;
          if constexpr (OP == OP_SRGB_TO_LAB)
            {
              double L,a,bb;
              xyz_to_lab(X,Y,Z,L,a,bb);
              o0=kQR*L; o1=kQR*a; o2=kQR*bb;
            }
          else
            {
              o0=kQR*X; o1=kQR*Y; o2=kQR*Z;
            }
          q[k][0]=QuantumOps<uint16_t>::clamp(o0);
          q[k][1]=QuantumOps<uint16_t>::clamp(o1);
          q[k][2]=QuantumOps<uint16_t>::clamp(o2);
          const size_t i=i0+(size_t) k*blockDim.x;
          if (i < npixels)
            store_pixel<uint16_t,C>(pixels+i*C,q[k]);
        }
    }
}

__global__ __launch_bounds__(1024)
void colorspace_lab_fast_kernel(uint4 *__restrict__ pairs,size_t npairs,uint2 *__restrict__ last)
{
  __shared__ float2 decode[kDecodePieces];
  build_decode_table(decode);
  __syncthreads();
  // two 8-byte pixels per lane and load; `last` is the odd pixel of the frame, if any
  constexpr int BATCH=4;
  const size_t stride=(size_t) gridDim.x*blockDim.x*BATCH;
  for (size_t i0=(size_t) blockIdx.x*blockDim.x*BATCH+threadIdx.x; i0 < npairs; i0+=stride)
    {
      uint4 v[BATCH];
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const size_t i=i0+(size_t) k*blockDim.x;
          v[k]=pairs[i < npairs ? i : npairs-1];
        }
#pragma unroll
      for (int k=0; k < BATCH; k++)
        {
          const uint2 first=srgb_to_lab_fast_pixel(make_uint2(v[k].x,v[k].y),decode);
          const uint2 second=srgb_to_lab_fast_pixel(make_uint2(v[k].z,v[k].w),decode);
          const size_t i=i0+(size_t) k*blockDim.x;
          if (i < npairs)
            pairs[i]=make_uint4(first.x,first.y,second.x,second.y);
        }
    }
  if ((last != nullptr) && (blockIdx.x == 0) && (threadIdx.x == 0))
    *last=srgb_to_lab_fast_pixel(*last,decode);
}

// ... on RGB frames (6-byte pixels, no alpha: what most photographs are; they took the table kernel of the bit-identical
// route at 2.8x the time of an RGBA frame): four pixels = three 8-byte words a lane; `tail` = the frame's last
// npixels mod 4 pixels.
__global__ __launch_bounds__(1024)
void colorspace_lab_fast_rgb_kernel(uint2 *__restrict__ words,size_t nquads,uint16_t *__restrict__ tail,int ntail)
{
  __shared__ float2 decode[kDecodePieces];
  build_decode_table(decode);
  __syncthreads();
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t i=(size_t) blockIdx.x*blockDim.x+threadIdx.x; i < nquads; i+=stride)
    {
      const uint2 w0=words[3*i],w1=words[3*i+1],w2=words[3*i+2];
      const uint2 p0=srgb_to_lab_fast_pixel(make_uint2(w0.x,w0.y & 0xffffu),decode);
      const uint2 p1=srgb_to_lab_fast_pixel(make_uint2((w0.y >> 16) | (w1.x << 16),w1.x >> 16),decode);
      const uint2 p2=srgb_to_lab_fast_pixel(make_uint2(w1.y,w2.x & 0xffffu),decode);
      const uint2 p3=srgb_to_lab_fast_pixel(make_uint2((w2.x >> 16) | (w2.y << 16),w2.y >> 16),decode);
      words[3*i]=make_uint2(p0.x,(p0.y & 0xffffu) | (p1.x << 16));
      words[3*i+1]=make_uint2((p1.x >> 16) | (p1.y << 16),p2.x);
      words[3*i+2]=make_uint2((p2.y & 0xffffu) | (p3.x << 16),(p3.x >> 16) | (p3.y << 16));
    }
  if ((blockIdx.x == 0) && ((int) threadIdx.x < ntail))
    {
      uint16_t *q=tail+3*threadIdx.x;
      const uint2 p=srgb_to_lab_fast_pixel(make_uint2((unsigned) q[0] | ((unsigned) q[1] << 16),(unsigned) q[2]),decode);
      q[0]=(uint16_t) (p.x & 0xffffu);
      q[1]=(uint16_t) (p.x >> 16);
      q[2]=(uint16_t) (p.y & 0xffffu);
    }
}

template<typename Q,int C,int OP>
__global__ __launch_bounds__(256)
void colorspace_kernel(Q *__restrict__ pixels,size_t npixels)
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
      Q (&q)[C]=qb[k];
      double r=(double) q[0],g=(double) q[1],b=(double) q[2];
      double o0,o1,o2;
      if constexpr (OP == OP_SRGB_TO_RGB)
        {
          o0=decode_pixel_gamma(r);
          o1=decode_pixel_gamma(g);
          o2=decode_pixel_gamma(b);
        }
      else if constexpr (OP == OP_RGB_TO_SRGB)
        {
          o0=encode_pixel_gamma(r);
          o1=encode_pixel_gamma(g);
          o2=encode_pixel_gamma(b);
        }
      else if constexpr (OP == OP_SRGB_TO_LAB)
        {
          double X,Y,Z,L,a,bb;
          rgb_to_xyz(r,g,b,X,Y,Z);
          xyz_to_lab(X,Y,Z,L,a,bb);
          o0=kQR*L; o1=kQR*a; o2=kQR*bb;          // colorspace.c:1041-1043
        }
      else if constexpr (OP == OP_SRGB_TO_XYZ)
        {
          double X,Y,Z;
          rgb_to_xyz(r,g,b,X,Y,Z);
          o0=kQR*X; o1=kQR*Y; o2=kQR*Z;
        }
      else if constexpr (OP == OP_LAB_TO_SRGB)
        {
          // ConvertGenericToRGB(QuantumScale*R,...) -> ConvertLabToRGB, colorspace.c:2373-2377
          double L=kQS*r,a=kQS*g,bb=kQS*b,X,Y,Z;
          lab_to_xyz(100.0*L,255.0*(a-0.5),255.0*(bb-0.5),X,Y,Z);
          xyz_to_rgb(X,Y,Z,o0,o1,o2);
        }
      else
        {
          xyz_to_rgb(kQS*r,kQS*g,kQS*b,o0,o1,o2);
        }
      q[0]=QuantumOps<Q>::clamp(o0);
      q[1]=QuantumOps<Q>::clamp(o1);
      q[2]=QuantumOps<Q>::clamp(o2);
      if (i < npixels)
        store_pixel<Q,C>(pixels+i*C,q);
    }
    }
}

template<typename Q,int C>
static MhStatus colorspace_typed(const View &img,int op)
{
  const size_t n=img.columns*img.rows;
  Q *p=static_cast<Q *>(img.pixels);
  dim3 grid(stream_grid((n+kPointBatch-1)/kPointBatch)),block(256);
  ProfileScope prof("colorspace",img.stream);
  switch (op)
  {
    case OP_SRGB_TO_RGB: hipLaunchKernelGGL((colorspace_kernel<Q,C,OP_SRGB_TO_RGB>),grid,block,0,img.stream,p,n); break;
    case OP_RGB_TO_SRGB: hipLaunchKernelGGL((colorspace_kernel<Q,C,OP_RGB_TO_SRGB>),grid,block,0,img.stream,p,n); break;
    case OP_SRGB_TO_LAB: hipLaunchKernelGGL((colorspace_kernel<Q,C,OP_SRGB_TO_LAB>),grid,block,0,img.stream,p,n); break;
    case OP_LAB_TO_SRGB: hipLaunchKernelGGL((colorspace_kernel<Q,C,OP_LAB_TO_SRGB>),grid,block,0,img.stream,p,n); break;
    case OP_SRGB_TO_XYZ: hipLaunchKernelGGL((colorspace_kernel<Q,C,OP_SRGB_TO_XYZ>),grid,block,0,img.stream,p,n); break;
    default: hipLaunchKernelGGL((colorspace_kernel<Q,C,OP_XYZ_TO_SRGB>),grid,block,0,img.stream,p,n); break;
  }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// per-device transfer-function tables (see colorspace_table_kernel); built on first use
struct ColorTables
{
  void *block=nullptr;
  double *decode_scaled=nullptr;
  uint16_t *decode_q16=nullptr,*encode_q16=nullptr;
};
static std::mutex color_tables_lock;
static std::map<int,ColorTables> color_tables;

static MhStatus acquire_color_tables(int device,hipStream_t stream,ColorTables *out)
{
  std::lock_guard<std::mutex> guard(color_tables_lock);
  auto it=color_tables.find(device);
  if (it != color_tables.end())
    {
      *out=it->second;
      return MH_OK;
    }
  ColorTables t;
  MH_HIP(hipMalloc(&t.block,65536*(sizeof(double)+2*sizeof(uint16_t))));
  t.decode_scaled=static_cast<double *>(t.block);
  t.decode_q16=reinterpret_cast<uint16_t *>(t.decode_scaled+65536);
  t.encode_q16=t.decode_q16+65536;
  hipLaunchKernelGGL(colorspace_table_kernel,dim3(256),dim3(256),0,stream,t.decode_scaled,
    t.decode_q16,t.encode_q16);
  hipError_t err=hipGetLastError();
  if (err == hipSuccess)
    err=hipStreamSynchronize(stream);      // once per device: other streams may use it next
  if (err != hipSuccess)
    {
      (void) hipFree(t.block);
      MH_HIP(err);
    }
  color_tables[device]=t;
  *out=t;
  return MH_OK;
}

void release_color_tables()
{
  std::lock_guard<std::mutex> guard(color_tables_lock);
  for (auto &kv : color_tables)
    (void) hipFree(kv.second.block);
  color_tables.clear();
}

static MhStatus colorspace_step(const View &img,int op)
{
  if ((op == OP_SRGB_TO_LAB) && (img.quantum == MH_QUANTUM_U16) && (img.channels == 4) &&
      (precision() == MH_PRECISION_FAST) && (option("MAGICKHIP_NO_FAST_LAB") == nullptr) &&
      ((reinterpret_cast<uintptr_t>(img.pixels) & 15u) == 0))
    {
      const size_t n=img.columns*img.rows,npairs=n/2;
      uint2 *last=(n & 1) != 0 ? static_cast<uint2 *>(img.pixels)+(n-1) : nullptr;
      if (npairs == 0)
        {
          hipLaunchKernelGGL(colorspace_lab_fast_kernel,dim3(1),dim3(1024),0,img.stream,
            static_cast<uint4 *>(img.pixels),(size_t) 0,last);
          MH_HIP(hipGetLastError());
          return MH_OK;
        }
      ProfileScope prof("colorspace",img.stream);
      // persistent workgroups, two per CU: each builds the decode table once
      const size_t wanted=(npairs+4095)/4096,most=2*(size_t) compute_units(img.device);
      hipLaunchKernelGGL(colorspace_lab_fast_kernel,dim3((unsigned) (wanted < most ? wanted : most)),dim3(1024),0,
        img.stream,static_cast<uint4 *>(img.pixels),npairs,last);
      MH_HIP(hipGetLastError());
      return MH_OK;
    }
  if ((op == OP_SRGB_TO_LAB) && (img.quantum == MH_QUANTUM_U16) && (img.channels == 3) &&
      (precision() == MH_PRECISION_FAST) && (option("MAGICKHIP_NO_FAST_LAB") == nullptr) &&
      ((reinterpret_cast<uintptr_t>(img.pixels) & 7u) == 0))
    {
      const size_t n=img.columns*img.rows,nquads=n/4;
      ProfileScope prof("colorspace",img.stream);
      const size_t wanted=(nquads+1023)/1024,most=2*(size_t) compute_units(img.device);
      hipLaunchKernelGGL(colorspace_lab_fast_rgb_kernel,dim3((unsigned) (wanted < 1 ? 1 : (wanted < most ? wanted : most))),
        dim3(1024),0,img.stream,static_cast<uint2 *>(img.pixels),nquads,
        static_cast<uint16_t *>(img.pixels)+12*nquads,(int) (n-4*nquads));
      MH_HIP(hipGetLastError());
      return MH_OK;
    }
  if ((img.quantum == MH_QUANTUM_U16) &&
      ((op == OP_SRGB_TO_RGB) || (op == OP_RGB_TO_SRGB) || (op == OP_SRGB_TO_LAB) ||
       (op == OP_SRGB_TO_XYZ)))
    {
      ColorTables t;
      MH_TRY(acquire_color_tables(img.device,img.stream,&t));
      if ((op == OP_SRGB_TO_RGB) || (op == OP_RGB_TO_SRGB))
        {
          // one 65536-entry Quantum column applied to the three colours
          Roles colours;
          colours.update_mask=0x7u;
          return launch_apply_lut(img,op == OP_SRGB_TO_RGB ? t.decode_q16 : t.encode_q16,0x7u,colours,-1,nullptr,true,
            "colorspace");
        }
      const size_t n=img.columns*img.rows;
      uint16_t *p=static_cast<uint16_t *>(img.pixels);
      dim3 grid(stream_grid((n+kPointBatch-1)/kPointBatch)),block(256);
      ProfileScope prof("colorspace",img.stream);
      dispatch_colour_layout(img.quantum,img.channels,[&](auto L) {
        if (op == OP_SRGB_TO_LAB)
          hipLaunchKernelGGL((colorspace_q16_table_kernel<L.C,OP_SRGB_TO_LAB>),grid,block,0,img.stream,p,n,t.decode_scaled);
        else
          hipLaunchKernelGGL((colorspace_q16_table_kernel<L.C,OP_SRGB_TO_XYZ>),grid,block,0,img.stream,p,n,t.decode_scaled); });
      MH_HIP(hipGetLastError());
      return MH_OK;
    }
  return dispatch_colour_layout(img.quantum,img.channels,[&](auto L) {
    return colorspace_typed<typename decltype(L)::Q,L.C>(img,op); });
}

// ---------------------------------------------------------------- the other pointwise colourspaces
static bool generic_colorspace(MhColorspace c)
{
  switch (c)
  {
    case MH_COLORSPACE_CMY: case MH_COLORSPACE_HCL: case MH_COLORSPACE_HCLP: case MH_COLORSPACE_HSB:
    case MH_COLORSPACE_HSI: case MH_COLORSPACE_HSL: case MH_COLORSPACE_HSV: case MH_COLORSPACE_HWB:
    case MH_COLORSPACE_LCH: case MH_COLORSPACE_LCHAB: case MH_COLORSPACE_LCHUV: case MH_COLORSPACE_LMS:
    case MH_COLORSPACE_LUV: case MH_COLORSPACE_XYY: case MH_COLORSPACE_YCBCR: case MH_COLORSPACE_YDBDR:
    case MH_COLORSPACE_YIQ: case MH_COLORSPACE_YPBPR: case MH_COLORSPACE_YUV: case MH_COLORSPACE_JZAZBZ:
    case MH_COLORSPACE_DISPLAYP3: case MH_COLORSPACE_ADOBE98: case MH_COLORSPACE_PROPHOTO:
    case MH_COLORSPACE_OKLAB: case MH_COLORSPACE_OKLCH: case MH_COLORSPACE_CAT02LMS:
      return true;
    default:
      return false;
  }
}

bool colorspace_is_accelerated(MhColorspace c)
{
  return (c == MH_COLORSPACE_SRGB) || (c == MH_COLORSPACE_RGB) || (c == MH_COLORSPACE_SCRGB) ||
    (c == MH_COLORSPACE_LAB) || (c == MH_COLORSPACE_XYZ) || generic_colorspace(c) ||
    (c == MH_COLORSPACE_OHTA) || (c == MH_COLORSPACE_REC601YCBCR) || (c == MH_COLORSPACE_REC709YCBCR) ||
    (c == MH_COLORSPACE_YCC) || (c == MH_COLORSPACE_LOG);
}

template<typename Q,int C>
static MhStatus colorspace_generic_typed(const View &img,MhColorspace colorspace,bool forward,
  double white_luminance)
{
  const size_t n=img.columns*img.rows;
  dim3 grid(stream_grid(n)),block(256);
  ProfileScope prof("colorspace",img.stream);
  if (forward)
    hipLaunchKernelGGL((colorspace_generic_kernel<Q,C,true>),grid,block,0,img.stream,
      static_cast<Q *>(img.pixels),n,(int) colorspace,white_luminance);
  else
    hipLaunchKernelGGL((colorspace_generic_kernel<Q,C,false>),grid,block,0,img.stream,
      static_cast<Q *>(img.pixels),n,(int) colorspace,white_luminance);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

static MhStatus colorspace_generic_step(const View &img,MhColorspace colorspace,bool forward)
{
  const double white_luminance=10000.0;          // colorspace.c:993 (no "white-luminance" property)
  return dispatch_colour_layout(img.quantum,img.channels,[&](auto L) {
    return colorspace_generic_typed<typename decltype(L)::Q,L.C>(img,colorspace,forward,white_luminance); });
}

// ---------------------------------------------------------------- the table-driven colourspaces
// OHTA, Rec601YCbCr, Rec709YCbCr and YCC are the half of sRGBTransformImage / TransformsRGBImage
// that works through three tables of MaxMap+1 TransformPackets (colorspace.c:1226-1420,
// :2560-2790): x_map[i], y_map[i], z_map[i] hold what map index i of the red, green and blue sample
// contributes to each result, the pixel loop adds the three entries (+ the primary offsets) and
// ScaleMapToQuantum rounds.  Every entry is ONE rounded product k*f(i) — f(i) = i (forward; the
// inverse's first table), 2i - MaxMap (inverse, second and third table: the constant 0.5*k is
// folded by the compiler as it would be multiplied), 1.099i - 0.099 (YCC above 0.018 MaxMap) — so
// the kernel forms the entries in place, in the table's own operations, instead of reading them.
// YCC -> sRGB goes through a 1389-entry film curve (YCCMap) and stays on the CPU.
struct MatrixColorspaceArgs
{
  double k[3][3];             // [table: red, green, blue index][result channel]
  double low[3][3];           // YCC forward: the entries of indices up to 0.018 MaxMap
  double primary[3];
  int form;                   // 0 forward, 1 inverse, 2 YCC forward
};

template<typename Q,int C>
__global__ __launch_bounds__(256)
void colorspace_matrix_kernel(Q *pixels,size_t npixels,MatrixColorspaceArgs a)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t at=(size_t) blockIdx.x*blockDim.x+threadIdx.x; at < npixels; at+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+at*C,q);
      double entry[3][3];
#pragma unroll
      for (int t=0; t < 3; t++)
        {
          // ScaleQuantumToMap(ClampToQuantum(sample)), colorspace.c:1459-1464, :2738-2740
          const unsigned index=QuantumOps<Q>::map_index(q[t]);
          const double i=(double) index;
          if (a.form == 2)
            {
              const bool low=index <= 1179u;      // (ssize_t) (0.018*MaxMap)
              const double upper=1.099*i-0.099;
#pragma unroll
              for (int c=0; c < 3; c++)
                entry[t][c]=low ? a.low[t][c]*i : a.k[t][c]*upper;
            }
          else
            {
              const double f=((a.form == 1) && (t != 0)) ? 2.0*i-65535.0 : i;
#pragma unroll
              for (int c=0; c < 3; c++)
                entry[t][c]=a.k[t][c]*f;
            }
        }
#pragma unroll
      for (int c=0; c < 3; c++)
        {
          double value=entry[0][c]+entry[1][c]+entry[2][c];
          if (a.form != 1)
            value=value+a.primary[c];
          // ScaleMapToQuantum, quantum-private.h:465-476
          if (value <= 0.0)
            q[c]=(Q) 0;
          else if (value >= 65535.0)
            q[c]=(Q) 65535;
          else
            q[c]=QuantumOps<Q>::is_float ? (Q) value : (Q) (value+0.5);
        }
      store_pixel<Q,C>(pixels+at*C,q);
    }
}

static bool matrix_colorspace(MhColorspace c)
{
  return (c == MH_COLORSPACE_OHTA) || (c == MH_COLORSPACE_REC601YCBCR) || (c == MH_COLORSPACE_REC709YCBCR) ||
    (c == MH_COLORSPACE_YCC);
}

static MhStatus colorspace_matrix_step(const View &img,MhColorspace colorspace,bool forward)
{
  MatrixColorspaceArgs a={};
  auto rows=[&](double (&to)[3][3],const double (&red)[3],const double (&green)[3],const double (&blue)[3])
  {
    for (int c=0; c < 3; c++)
      {
        to[0][c]=red[c];
        to[1][c]=green[c];
        to[2][c]=blue[c];
      }
  };
  a.form=forward ? 0 : 1;
  if (forward)
    {
      a.primary[0]=0.0;
      a.primary[1]=a.primary[2]=32768.0;          // (MaxMap+1)/2
    }
  switch (colorspace)
  {
    case MH_COLORSPACE_OHTA:
      if (forward)
        rows(a.k,{0.33333,0.50000,-0.25000},{0.33334,0.00000,0.50000},{0.33333,-0.50000,-0.25000});
      else
        rows(a.k,{1.0,1.0,1.0},{0.5*1.00000,0.5*0.00000,-0.5*1.00000},{-0.5*0.66668,0.5*1.33333,-0.5*0.66668});
      break;
    case MH_COLORSPACE_REC601YCBCR:
      if (forward)
        rows(a.k,{0.298839,-0.1687367,0.500000},{0.586811,-0.331264,-0.418688},{0.114350,0.500000,-0.081312});
      else
        rows(a.k,{0.99999999999914679361,0.99999975910502514331,1.00000124040004623180},
          {0.5*(-1.2188941887145875e-06),0.5*(-0.34413567816504303521),0.5*1.77200006607230409200},
          {0.5*1.4019995886561440468,0.5*(-0.71413649331646789076),0.5*2.1453384174593273e-06});
      break;
    case MH_COLORSPACE_REC709YCBCR:
      if (forward)
        rows(a.k,{0.212656,-0.114572,0.500000},{0.715158,-0.385428,-0.454153},{0.072186,0.500000,-0.045847});
      else
        rows(a.k,{1.0,1.0,1.0},{0.5*0.000000,0.5*(-0.187324),0.5*1.855600},{0.5*1.574800,0.5*(-0.468124),0.5*0.000000});
      break;
    case MH_COLORSPACE_YCC:
      if (!forward)
        return fail(MH_UNSUPPORTED,"YCC -> sRGB (the YCCMap film curve) is not accelerated");
      a.form=2;
      rows(a.low,{0.005382,-0.003296,0.009410},{0.010566,-0.006471,-0.007880},{0.002052,0.009768,-0.001530});
      rows(a.k,{0.298839,-0.298839,0.70100},{0.586811,-0.586811,-0.586811},{0.114350,0.88600,-0.114350});
      a.primary[1]=40092.0;                        // ScaleQuantumToMap(ScaleCharToQuantum(156))
      a.primary[2]=35209.0;                        // ... (137)
      break;
    default:
      return fail(MH_UNSUPPORTED,"colourspace %d is not table-driven",(int) colorspace);
  }
  const size_t n=img.columns*img.rows;
  dim3 grid(stream_grid(n)),block(256);
  ProfileScope prof("colorspace",img.stream);
  dispatch_colour_layout(img.quantum,img.channels,[&](auto L) {
    using Q=typename decltype(L)::Q;
    hipLaunchKernelGGL((colorspace_matrix_kernel<Q,L.C>),grid,block,0,img.stream,static_cast<Q *>(img.pixels),n,a); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// Log (Cineon film density, colorspace.c:1055-1163, :2391-2501): a table of MaxMap+1 Quantum values
// built from four film parameters — here with their defaults (the image properties "gamma",
// "film-gamma", "reference-black", "reference-white" change them: the caller declines then) —
// indexed by the DECODED sample on the way in, and followed by EncodePixelGamma on the way back.
// The table is built on the host in the reference's own expressions (libm's pow and log10).
template<typename Q>
static void build_log_table(bool forward,std::vector<Q> &table)
{
  const double density=1.0/1.7,gamma=1.0/1.7,film_gamma=0.6,reference_black=95.0,reference_white=685.0;
  const double max_map=65535.0;
  // PerceptibleReciprocal (pixel-accessor.h: 1/x, clamped at MagickEpsilon)
  auto reciprocal=[](double x) { const double sign=x < 0.0 ? -1.0 : 1.0; return (sign*x) >= 1.0e-12 ? 1.0/x : sign/1.0e-12; };
  auto map_to_quantum=[&](double value) -> Q    // ScaleMapToQuantum, quantum-private.h:465-476
  {
    if (value <= 0.0)
      return (Q) 0;
    if (value >= max_map)
      return (Q) 65535;
    return std::is_same<Q,float>::value ? (Q) value : (Q) (value+0.5);
  };
  table.assign(65536,(Q) 0);
  const double black=std::pow(10.0,(reference_black-reference_white)*(gamma/density)*0.002*reciprocal(film_gamma));
  if (forward)
    {
      for (long i=0; i <= 65535; i++)
        table[(size_t) i]=map_to_quantum((max_map*(reference_white+std::log10(black+(1.0*(double) i/max_map)*(1.0-black))/
          ((gamma/density)*0.002*reciprocal(film_gamma)))/1024.0));
      return;
    }
  long i=0;
  for ( ; i <= (long) (reference_black*max_map/1024.0); i++)
    table[(size_t) i]=(Q) 0;
  for ( ; i < (long) (reference_white*max_map/1024.0); i++)
    {
      const double value=65535.0/(1.0-black)*(std::pow(10.0,(1024.0*(double) i/max_map-reference_white)*(gamma/density)*0.002*
        reciprocal(film_gamma))-black);
      // ClampToQuantum (quantum.h:86-97)
      if (std::is_same<Q,float>::value)
        table[(size_t) i]=(Q) value;
      else
        table[(size_t) i]=!(value > 0.0) ? (Q) 0 : (value >= 65535.0 ? (Q) 65535 : (Q) (value+0.5));
    }
  for ( ; i <= 65535; i++)
    table[(size_t) i]=(Q) 65535;
}

template<typename Q,int C,bool FORWARD>
__global__ __launch_bounds__(256)
void colorspace_log_kernel(Q *pixels,size_t npixels,const Q *table)
{
  const size_t stride=(size_t) gridDim.x*blockDim.x;
  for (size_t at=(size_t) blockIdx.x*blockDim.x+threadIdx.x; at < npixels; at+=stride)
    {
      Q q[C];
      load_pixel<Q,C>(pixels+at*C,q);
#pragma unroll
      for (int c=0; c < 3; c++)
        {
          if constexpr (FORWARD)
            q[c]=table[QuantumOps<Q>::map_index(QuantumOps<Q>::clamp(decode_pixel_gamma((double) q[c])))];
          else
            q[c]=QuantumOps<Q>::clamp(encode_pixel_gamma((double) table[QuantumOps<Q>::map_index(q[c])]));
        }
      store_pixel<Q,C>(pixels+at*C,q);
    }
}

template<typename Q,int C>
static MhStatus colorspace_log_typed(const View &img,bool forward)
{
  std::vector<Q> host;
  build_log_table<Q>(forward,host);
  Temp table;
  MH_TRY(upload_table(table,img.device,img.stream,host.data(),host.size()*sizeof(Q)));
  const size_t n=img.columns*img.rows;
  dim3 grid(stream_grid(n)),block(256);
  Q *pixels=static_cast<Q *>(img.pixels);
  ProfileScope prof("colorspace",img.stream);
  if (forward)
    hipLaunchKernelGGL((colorspace_log_kernel<Q,C,true>),grid,block,0,img.stream,pixels,n,table.as<Q>());
  else
    hipLaunchKernelGGL((colorspace_log_kernel<Q,C,false>),grid,block,0,img.stream,pixels,n,table.as<Q>());
  MH_HIP(hipGetLastError());
  return MH_OK;
}

static bool colorspace_is_generic(MhColorspace c)
{
  return generic_colorspace(c) || matrix_colorspace(c) || (c == MH_COLORSPACE_LOG);
}
static MhStatus colorspace_generic_forward_or_inverse(const View &img,MhColorspace colorspace,bool forward)
{
  if (colorspace == MH_COLORSPACE_LOG)
    return dispatch_colour_layout(img.quantum,img.channels,[&](auto L) {
      return colorspace_log_typed<typename decltype(L)::Q,L.C>(img,forward); });
  if (matrix_colorspace(colorspace))
    return colorspace_matrix_step(img,colorspace,forward);
  return colorspace_generic_step(img,colorspace,forward);
}

MhStatus launch_colorspace(const View &img,MhColorspace from,MhColorspace to,const MhImage *)
{
  if ((img.channels != 3) && (img.channels != 4))
    return fail(MH_UNSUPPORTED,"colourspace transform needs R,G,B[,A] channels");
  // TransformImageColorspace, colorspace.c:1751-1783: X -> sRGB -> Y
  if (from != MH_COLORSPACE_SRGB)
    {
      int op=-1;
      switch (from)
      {
        case MH_COLORSPACE_RGB: case MH_COLORSPACE_SCRGB: op=OP_RGB_TO_SRGB; break;   // (one case: colorspace.c:2502-2503)
        case MH_COLORSPACE_LAB: op=OP_LAB_TO_SRGB; break;
        case MH_COLORSPACE_XYZ: op=OP_XYZ_TO_SRGB; break;
        default:
          if (!colorspace_is_generic(from))
            return fail(MH_UNSUPPORTED,"source colourspace %d is not accelerated",(int) from);
          break;
      }
      if (op >= 0)
        MH_TRY(colorspace_step(img,op));
      else
        MH_TRY(colorspace_generic_forward_or_inverse(img,from,false));
    }
  if (to != MH_COLORSPACE_SRGB)
    {
      int op=-1;
      switch (to)
      {
        case MH_COLORSPACE_RGB: case MH_COLORSPACE_SCRGB: op=OP_SRGB_TO_RGB; break;   // (colorspace.c:1164-1165)
        case MH_COLORSPACE_LAB: op=OP_SRGB_TO_LAB; break;
        case MH_COLORSPACE_XYZ: op=OP_SRGB_TO_XYZ; break;
        default:
          if (!colorspace_is_generic(to))
            return fail(MH_UNSUPPORTED,"target colourspace %d is not accelerated",(int) to);
          break;
      }
      if (op >= 0)
        MH_TRY(colorspace_step(img,op));
      else
        MH_TRY(colorspace_generic_forward_or_inverse(img,to,true));
    }
  return MH_OK;
}

MhStatus launch_modulate_generic(const View &img,MhColorspace colorspace,double hue_shift,
  double saturation_scale,double brightness_scale)
{
  if ((img.channels != 3) && (img.channels != 4))
    return fail(MH_UNSUPPORTED,"modulate needs R,G,B[,A] channels");
  const size_t n=img.columns*img.rows;
  dim3 grid(stream_grid(n)),block(256);
  ProfileScope prof("modulate",img.stream);
  dispatch_colour_layout(img.quantum,img.channels,[&](auto L) {
    using Q=typename decltype(L)::Q;
    hipLaunchKernelGGL((modulate_generic_kernel<Q,L.C>),grid,block,0,img.stream,static_cast<Q *>(img.pixels),n,
      (int) colorspace,hue_shift,saturation_scale,brightness_scale); });
  MH_HIP(hipGetLastError());
  return MH_OK;
}

} // namespace mh
