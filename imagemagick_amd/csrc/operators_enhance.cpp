// In-place operators: ContrastStretchImage, EqualizeImage,
// TransformImageColorspace, and the histogram / LUT building blocks they are
// made of (exposed so a row-sharded image can all-reduce the histogram between
// the phases — SURVEY §8e).
//
// The histogram and the LUT application are HIP kernels (histogram.hip); the
// 65536-entry scans that turn a histogram into a LUT are restated here on the
// host from MagickCore/enhance.c:1652-1706 (contrast stretch) and :2138-2169
// (equalize), in the reference's arithmetic.
#include "mh_internal.hpp"

#include <cmath>
#include <cstring>
#include <mutex>

namespace mh {

static double perceptible_reciprocal(double x)
{
  double sign=x < 0.0 ? -1.0 : 1.0;
  if ((sign*x) >= kMagickEpsilon)
    return 1.0/x;
  return sign/kMagickEpsilon;
}

// ScaleMapToQuantum, quantum-private.h:465-476, result as the Quantum it
// would be stored in (unsigned short or float), widened to double
static double scale_map_to_quantum(double value,MhQuantumKind quantum)
{
  if (value <= 0.0)
    return 0.0;
  if (value >= (double) MH_MAXMAP)
    return kQuantumRange;
  if (quantum == MH_QUANTUM_U16)
    return (double) (unsigned short) (value+0.5);
  return (double) (float) value;
}

struct InPlace
{
  DeviceGuard guard;         // declared first: the device is restored after img is gone
  Resident img;
  MhStatus open(MhImage *image)
  {
    int device=resolve_device(image);
    hipStream_t stream=image->memory == MH_MEMORY_DEVICE ? (hipStream_t) image->stream :
      library_stream(device);
    MH_TRY(img.open(image,2,stream,device));
    img.view.stream=stream;
    img.view.device=device;
    MH_HIP(guard.enter(device));
    return MH_OK;
  }
};

static MhStatus check_image(const MhImage *image,const char *what)
{
  MH_TRY(runtime_ready());
  MH_TRY(validate_image(image,what));
  set_call_precision(image);       // MhImage::precision of this call, else the library default
  return MH_OK;
}

// device histogram -> host
static MhStatus histogram_to_host(const View &view,int mode,const MhImage *desc,
  std::vector<unsigned long long> &host)
{
  const size_t n=(size_t) MH_HISTOGRAM_BINS*(size_t) view.channels;
  Temp hist;
  MH_TRY(hist.alloc(view.device,n*sizeof(unsigned long long),view.stream));
  MH_HIP(hipMemsetAsync(hist.ptr,0,n*sizeof(unsigned long long),view.stream));
  MH_TRY(launch_histogram(view,mode,desc,hist.as<unsigned long long>()));
  host.resize(n);
  MH_HIP(hipMemcpyAsync(host.data(),hist.ptr,n*sizeof(unsigned long long),
    hipMemcpyDeviceToHost,view.stream));
  MH_HIP(hipStreamSynchronize(view.stream));
  return MH_OK;
}

// LUT (double, Quantum-valued) -> device LUT in the image's Quantum type -> apply
static MhStatus apply_lut_host(const View &view,const MhImage *desc,const double *lut,
  uint32_t apply_mask)
{
  const size_t n=(size_t) MH_HISTOGRAM_BINS*(size_t) view.channels;
  Temp d_lut;
  int shared_column=-1;
  if (view.quantum == MH_QUANTUM_U16)
    {
      std::vector<unsigned short> q(n);
      for (size_t i=0; i < n; i++)
        {
          // ClampToQuantum of a value that already is a Quantum
          double v=lut[i];
          q[i]=(unsigned short) (!(v > 0.0) ? 0 : (v >= kQuantumRange ? 65535 : (unsigned short) (v+0.5)));
        }
      // do all selected channels share one column?
      const int C=view.channels;
      int first=-1;
      bool same=true;
      for (int c=0; (c < C) && same; c++)
        {
          if (((apply_mask >> c) & 1u) == 0)
            continue;
          if (first < 0)
            {
              first=c;
              continue;
            }
          for (size_t b=0; b < (size_t) MH_HISTOGRAM_BINS; b++)
            if (q[b*(size_t) C+(size_t) c] != q[b*(size_t) C+(size_t) first])
              {
                same=false;
                break;
              }
        }
      if (same && (first >= 0))
        shared_column=first;
      MH_TRY(upload_table(d_lut,view.device,view.stream,q.data(),n*sizeof(unsigned short)));
    }
  else
    {
      std::vector<float> q(n);
      for (size_t i=0; i < n; i++)
        q[i]=(float) lut[i];
      MH_TRY(upload_table(d_lut,view.device,view.stream,q.data(),n*sizeof(float)));
    }
  Roles roles=channel_roles(desc,desc);
  // enhance.c:1781, :2255: only channels whose traits carry Update
  uint32_t update=0;
  for (uint32_t c=0; c < desc->number_channels; c++)
    if ((desc->channel_traits[c] & MH_TRAIT_UPDATE) != 0)
      update|=1u<<c;
  roles.update_mask=update;
  return launch_apply_lut(view,d_lut.ptr,apply_mask,roles,shared_column);
}

// histogram [65536][channels] on the device -> LUT -> apply, all on the stream (the second
// half of ContrastStretchImage / EqualizeImage; MagickHipShardedImage calls it with a table
// that was all-reduced over the row bands of one image)
MhStatus apply_histogram_lut(const View &view,const MhImage *image,const unsigned long long *hist,
  int mode,bool equalize,double black_point,double white_limit,const unsigned int *colour_flag)
{
  if (!equalize && (view.channels <= 4) && (option("MAGICKHIP_NO_STRETCH_LEVELS") == nullptr))
    {
      // ContrastStretchImage: the levels of every channel, then the map evaluated per sample — no
      // table to build and gather from (histogram.hip)
      uint32_t update=0;
      for (uint32_t c=0; c < image->number_channels; c++)
        if ((image->channel_traits[c] & MH_TRAIT_UPDATE) != 0)
          update|=1u<<c;
      return launch_stretch_levels_apply(view,hist,black_point,white_limit,update,colour_flag);
    }
  const size_t n=(size_t) MH_HISTOGRAM_BINS*(size_t) view.channels;
  Temp lut,mask;
  MH_TRY(lut.alloc(view.device,n*(view.quantum == MH_QUANTUM_U16 ? sizeof(unsigned short) :
    sizeof(float)),view.stream));
  MH_TRY(mask.alloc(view.device,sizeof(uint32_t),view.stream));
  Roles roles=channel_roles(image,image);
  // enhance.c:1781, :2255: only channels whose traits carry Update
  uint32_t update=0;
  for (uint32_t c=0; c < image->number_channels; c++)
    if ((image->channel_traits[c] & MH_TRAIT_UPDATE) != 0)
      update|=1u<<c;
  roles.update_mask=update;
  // intensity binning gives every channel the same histogram, hence the same LUT column
  int shared_column=-1;
  if (((mode != 0) || (view.channels == 1)) && (update != 0))
    shared_column=__builtin_ctz(update);
  // EqualizeImage on a float frame: the map evaluated per sample from the running counts in LDS
  // instead of gathered from a 65536-float table (histogram.hip)
  if (equalize && (view.quantum != MH_QUANTUM_U16) && (shared_column >= 0) && (view.channels <= 4) &&
      (view.columns*view.rows >= ((size_t) 1 << 20)) && (option("MAGICKHIP_NO_EQUALIZE_COUNTS") == nullptr))
    {
      Temp counts;
      MH_TRY(counts.alloc(view.device,(size_t) MH_HISTOGRAM_BINS*sizeof(uint32_t),view.stream));
      MH_TRY(launch_build_lut(view,hist,equalize,black_point,white_limit,
        lut.ptr,mask.as<uint32_t>(),colour_flag,counts.as<uint32_t>(),shared_column));
      return launch_equalize_cdf_apply(view,counts.as<uint32_t>(),lut.ptr,~0u,roles,shared_column,mask.as<uint32_t>());
    }
  MH_TRY(launch_build_lut(view,hist,equalize,black_point,white_limit,
    lut.ptr,mask.as<uint32_t>(),colour_flag));
  return launch_apply_lut(view,lut.ptr,~0u,roles,shared_column,mask.as<uint32_t>());
}

// ------------------------------------------------------------------ the level operators
// (MagickCore/enhance.c: LevelImage :2913, LevelizeImage :3062, GammaImage :2322, NegateImage :3940,
// SigmoidalContrastImage :4267, LinearStretchImage :3347; MinMaxStretchImage histogram.c:927)
static uint32_t update_mask_of(const MhImage *image)
{
  uint32_t update=0;
  for (uint32_t c=0; c < image->number_channels; c++)
    if ((image->channel_traits[c] & MH_TRAIT_UPDATE) != 0)
      update|=1u<<c;
  return update;
}

// ClampToQuantum of the Quantum type, widened to double
static double clamp_to_quantum(double value,MhQuantumKind quantum)
{
  if (quantum != MH_QUANTUM_U16)
    return (double) (float) value;
  if (!(value > 0.0))
    return 0.0;
  if (value >= kQuantumRange)
    return kQuantumRange;
  return (double) (unsigned short) (value+0.5);
}

// gamma_pow, enhance.c:2317-2320
static double gamma_pow(double value,double gamma)
{
  return value < 0.0 ? value : pow(value,gamma);
}

// A curve that calls libm, tabulated over the 65536 Q16 samples with the host's libm (the one the
// reference links), Quantum-typed.  A few tables are kept per process, keyed by curve and
// parameters: a batch with one parameter set builds its table once.
enum { LEVELS_TABLE_LEVEL=0,LEVELS_TABLE_LEVELIZE=1,LEVELS_TABLE_SIGMOIDAL=2,LEVELS_TABLE_SIGMOIDAL_INVERSE=3,
  LEVELS_TABLE_GAMMA=4 };
struct LevelsTable
{
  int curve;
  MhQuantumKind quantum;
  double p[4];
  std::shared_ptr<const std::vector<unsigned char>> column;
};
static std::mutex &levels_tables_lock() { static std::mutex &m=*new std::mutex; return m; }
static std::vector<LevelsTable> &levels_tables() { static std::vector<LevelsTable> &v=*new std::vector<LevelsTable>; return v; }
static unsigned long long levels_tables_built=0;

static double levels_curve(int curve,const double *p,double q)
{
  switch (curve)
  {
    case LEVELS_TABLE_LEVEL:
      return kQuantumRange*gamma_pow(p[0]*(q-p[1]),p[2]);
    case LEVELS_TABLE_LEVELIZE:
      return gamma_pow(kQuantumScale*q,p[2])*p[0]+p[1];
    case LEVELS_TABLE_SIGMOIDAL:
      return kQuantumRange*((tanh(p[0]*(kQuantumScale*q-p[1]))-p[2])/(p[3]-p[2]));
    default:
      break;
  }
  const double argument=(p[3]-p[2])*(kQuantumScale*q)+p[2];
  const double clamped=argument < -1+kMagickEpsilon ? -1+kMagickEpsilon :
    (argument > 1-kMagickEpsilon ? 1-kMagickEpsilon : argument);
  return kQuantumRange*(p[1]+p[0]*atanh(clamped));
}

static std::shared_ptr<const std::vector<unsigned char>> levels_table(int curve,MhQuantumKind quantum,
  const double *p)
{
  constexpr size_t kTables=16;
  std::lock_guard<std::mutex> guard(levels_tables_lock());
  std::vector<LevelsTable> &tables=levels_tables();
  for (size_t i=0; i < tables.size(); i++)
    if ((tables[i].curve == curve) && (tables[i].quantum == quantum) &&
        (memcmp(tables[i].p,p,sizeof(tables[i].p)) == 0))
      {
        LevelsTable hit=std::move(tables[i]);
        tables.erase(tables.begin()+(ptrdiff_t) i);
        tables.insert(tables.begin(),std::move(hit));
        return tables[0].column;
      }
  const size_t size=quantum == MH_QUANTUM_U16 ? sizeof(unsigned short) : sizeof(float);
  auto column=std::make_shared<std::vector<unsigned char>>((size_t) MH_HISTOGRAM_BINS*size);
  if (curve == LEVELS_TABLE_GAMMA)
    {
      std::vector<double> lut((size_t) MH_HISTOGRAM_BINS);
      (void) MhGammaLUT(p[0],quantum,lut.data());
      for (size_t i=0; i <= MH_MAXMAP; i++)
        if (quantum == MH_QUANTUM_U16)
          reinterpret_cast<unsigned short *>(column->data())[i]=(unsigned short) lut[i];
        else
          reinterpret_cast<float *>(column->data())[i]=(float) lut[i];
    }
  else
    for (size_t i=0; i <= MH_MAXMAP; i++)
      {
        // LevelImage ends in ClampImage, which leaves a Q16 sample as it is
        const double value=clamp_to_quantum(levels_curve(curve,p,(double) i),quantum);
        if (quantum == MH_QUANTUM_U16)
          reinterpret_cast<unsigned short *>(column->data())[i]=(unsigned short) value;
        else
          reinterpret_cast<float *>(column->data())[i]=(float) value;
      }
  levels_tables_built++;
  LevelsTable entry;
  entry.curve=curve;
  entry.quantum=quantum;
  memcpy(entry.p,p,sizeof(entry.p));
  entry.column=column;
  tables.insert(tables.begin(),std::move(entry));
  if (tables.size() > kTables)
    tables.pop_back();
  return column;
}

// one tabulated curve applied to the channels of `update`
static MhStatus apply_levels_table(const View &view,int curve,const double *p,uint32_t update,const char *label)
{
  if ((update == 0) || (view.columns == 0) || (view.rows == 0))
    return MH_OK;
  const std::shared_ptr<const std::vector<unsigned char>> column=levels_table(curve,view.quantum,p);
  const void *device_column=nullptr;
  std::shared_ptr<void> keep;
  MH_TRY(shared_table(view.device,view.stream,column->data(),column->size(),&device_column,&keep));
  Roles roles;
  roles.update_mask=update;
  return launch_apply_lut(view,device_column,update,roles,0,nullptr,true,label);
}

// LevelImage on an open frame, the channels of `update`
static MhStatus level_view(const View &view,uint32_t update,double black_point,double white_point,double gamma)
{
  const double scale=perceptible_reciprocal(white_point-black_point);
  const double exponent=perceptible_reciprocal(gamma);
  if ((exponent != 1.0) && (view.quantum == MH_QUANTUM_U16))
    {
      const double p[4]={scale,black_point,exponent,0.0};
      return apply_levels_table(view,LEVELS_TABLE_LEVEL,p,update,"levels_level_table");
    }
  LevelsParams params;
  params.mode=exponent != 1.0 ? MH_LEVELS_LEVEL_POW : MH_LEVELS_LEVEL;    // pow(v,1.0) is v
  params.update_mask=update;
  params.a=scale;
  params.b=black_point;
  params.c=exponent;
  return launch_levels_point(view,params);
}

// the ten words of launch_levels_range on the host
static MhStatus range_to_host(const View &view,bool column0_only,double *slots)
{
  constexpr size_t bytes=2*(MH_MAX_CHANNELS+1)*sizeof(double);
  Temp result;
  MH_TRY(result.alloc(view.device,bytes,view.stream));
  MH_TRY(launch_levels_range(view,column0_only,result.as<double>()));
  MH_HIP(hipMemcpyAsync(slots,result.ptr,bytes,hipMemcpyDeviceToHost,view.stream));
  MH_HIP(hipStreamSynchronize(view.stream));
  return MH_OK;
}

// GetImageRange, statistic.c:1851-1929: every row starts from p[0], the offset-0 sample of its
// first pixel, whatever the mask, so the range is over the channels of `update` and column 0 of
// channel 0; *maxima starts at MagickMinimumValue and *minima at MagickMaximumValue
static void combine_range(const double *slots,const View &view,uint32_t update,double *minimum,double *maximum)
{
  *maximum=2.22507385850720140E-308;
  *minimum=1.79769313486231570E+308;
  if ((view.columns == 0) || (view.rows == 0))
    return;
  for (int c=0; c <= MH_MAX_CHANNELS; c++)
    {
      if ((c < MH_MAX_CHANNELS) && (((update >> c) & 1u) == 0))
        continue;
      if (slots[2*c] < *minimum)
        *minimum=slots[2*c];
      if (slots[2*c+1] > *maximum)
        *maximum=slots[2*c+1];
    }
}

// MinMaxStretchImage on an open frame, histogram.c:927-975
static MhStatus min_max_stretch_view(const View &view,const MhImage *image,double black,double white,double gamma)
{
  const uint32_t update=update_mask_of(image);
  double slots[2*(MH_MAX_CHANNELS+1)],minimum,maximum;
  MH_TRY(range_to_host(view,false,slots));
  if (image->channel_mask == MH_ALL_CHANNELS)
    {
      combine_range(slots,view,update,&minimum,&maximum);
      minimum+=black;
      maximum-=white;
      if (fabs(minimum-maximum) >= kMagickEpsilon)
        MH_TRY(level_view(view,update,minimum,maximum,gamma));
      return MH_OK;
    }
  // Per channel, in the order of the offsets.  The mask of offset i is the ChannelType bit 1 << i
  // (histogram.c:966), which names the channel stored there unless that channel is alpha (bit 4):
  // for the alpha offset no stored channel is selected, the range is the seed alone and nothing is
  // levelled.  Levelling channel 0 changes column 0 of channel 0, the seed of the later ranges.
  for (uint32_t i=0; i < image->number_channels; i++)
    {
      if (((update >> i) & 1u) == 0)
        continue;
      const uint32_t selected=(int32_t) i == image->alpha_offset ? 0u : 1u<<i;
      combine_range(slots,view,selected,&minimum,&maximum);
      minimum+=black;
      maximum-=white;
      if ((selected == 0) || !(fabs(minimum-maximum) >= kMagickEpsilon))
        continue;
      MH_TRY(level_view(view,selected,minimum,maximum,gamma));
      if ((i == 0) && (image->number_channels > 1))
        {
          double seed[2*(MH_MAX_CHANNELS+1)];
          MH_TRY(range_to_host(view,true,seed));
          slots[2*MH_MAX_CHANNELS]=seed[2*MH_MAX_CHANNELS];
          slots[2*MH_MAX_CHANNELS+1]=seed[2*MH_MAX_CHANNELS+1];
        }
    }
  return MH_OK;
}

} // namespace mh

using namespace mh;

extern "C" {

MH_API MhStatus MhContrastStretchLUT(const uint64_t *histogram,uint32_t number_channels,
  size_t columns,size_t rows,double black_point,double white_point,MhQuantumKind quantum,
  double *lut,uint32_t *apply_mask)
{
  if ((histogram == nullptr) || (lut == nullptr) || (number_channels == 0) ||
      (number_channels > MH_MAX_CHANNELS))
    return fail(MH_BAD_ARGUMENT,"ContrastStretchLUT: bad arguments");
  const size_t C=number_channels;
  uint32_t mask=0;
  memset(lut,0,(size_t) MH_HISTOGRAM_BINS*C*sizeof(double));
  for (size_t i=0; i < C; i++)
    {
      // locate the black/white levels, enhance.c:1652-1678.  black[] / white[]
      // are Quantum-typed in the reference; the indices fit either kind exactly.
      double intensity=0.0;
      ptrdiff_t j;
      for (j=0; j <= (ptrdiff_t) MH_MAXMAP; j++)
        {
          intensity+=(double) histogram[C*(size_t) j+i];
          if (intensity > black_point)
            break;
        }
      // black[i]=(Quantum) j, enhance.c:1668: when no bin exceeds black_point the scan ends with
      // j = MaxMap+1, which the Q16 build stores as (unsigned short) 65536 = 0
      const double black=quantum == MH_QUANTUM_U16 ? (double) (j & 0xffff) : (double) j;
      intensity=0.0;
      for (j=(ptrdiff_t) MH_MAXMAP; j != 0; j--)
        {
          intensity+=(double) histogram[C*(size_t) j+i];
          if (intensity > ((double) columns*(double) rows-white_point))
            break;
        }
      const double white=(double) j;
      // stretch map, enhance.c:1685-1706
      for (j=0; j <= (ptrdiff_t) MH_MAXMAP; j++)
        {
          double gamma=perceptible_reciprocal(white-black);
          if (j < (ptrdiff_t) black)
            lut[C*(size_t) j+i]=0.0;
          else if (j > (ptrdiff_t) white)
            lut[C*(size_t) j+i]=kQuantumRange;
          else if (black != white)
            lut[C*(size_t) j+i]=scale_map_to_quantum(
              (double) ((double) MH_MAXMAP*gamma*((double) j-black)),quantum);
        }
      if (black != white)
        mask|=1u<<i;
    }
  if (apply_mask != nullptr)
    *apply_mask=mask;
  return MH_OK;
}

MH_API MhStatus MhEqualizeLUT(const uint64_t *histogram,uint32_t number_channels,
  MhQuantumKind quantum,double *lut,uint32_t *apply_mask)
{
  if ((histogram == nullptr) || (lut == nullptr) || (number_channels == 0) ||
      (number_channels > MH_MAX_CHANNELS))
    return fail(MH_BAD_ARGUMENT,"EqualizeLUT: bad arguments");
  const size_t C=number_channels;
  uint32_t mask=0;
  std::vector<double> map((size_t) MH_HISTOGRAM_BINS);
  memset(lut,0,(size_t) MH_HISTOGRAM_BINS*C*sizeof(double));
  for (size_t i=0; i < C; i++)
    {
      // integrate, enhance.c:2138-2152
      double intensity=0.0;
      for (size_t j=0; j <= MH_MAXMAP; j++)
        {
          intensity+=(double) histogram[C*j+i];
          map[j]=intensity;
        }
      const double black=map[0],white=map[MH_MAXMAP];
      if (black != white)
        {
          // enhance.c:2162-2168
          for (size_t j=0; j <= MH_MAXMAP; j++)
            lut[C*j+i]=scale_map_to_quantum(
              (double) (((double) MH_MAXMAP*(map[j]-black))/(white-black)),quantum);
          mask|=1u<<i;
        }
    }
  if (apply_mask != nullptr)
    *apply_mask=mask;
  return MH_OK;
}

MH_API MhStatus MagickHipHistogram(const MhImage *image,int intensity_mode,uint64_t *histogram)
{
  MH_TRY(check_image(image,"Histogram"));
  if (histogram == nullptr)
    return fail(MH_BAD_ARGUMENT,"Histogram: null histogram");
  const size_t n=(size_t) MH_HISTOGRAM_BINS*(size_t) image->number_channels;
  DeviceGuard guard;
  if (image->memory == MH_MEMORY_DEVICE)
    {
      Resident img;
      MH_TRY(img.open(image,0,nullptr,-1));
      MH_HIP(guard.enter(img.view.device));
      return launch_histogram(img.view,intensity_mode,image,
        reinterpret_cast<unsigned long long *>(histogram));
    }
  Resident img;
  int device=resolve_device(image);
  MH_TRY(img.open(image,0,library_stream(device),device));
  MH_HIP(guard.enter(device));
  std::vector<unsigned long long> host;
  MH_TRY(histogram_to_host(img.view,intensity_mode,image,host));
  for (size_t i=0; i < n; i++)
    histogram[i]+=host[i];
  return img.commit();
}

MH_API MhStatus MagickHipApplyLUT(MhImage *image,const double *lut,uint32_t apply_mask)
{
  MH_TRY(check_image(image,"ApplyLUT"));
  if (lut == nullptr)
    return fail(MH_BAD_ARGUMENT,"ApplyLUT: null LUT");
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(apply_lut_host(io.img.view,image,lut,apply_mask));
  return io.img.commit();
}

MH_API MhStatus MagickHipIsImageGray(const MhImage *image,int *is_gray)
{
  MH_TRY(check_image(image,"IsImageGray"));
  if (is_gray == nullptr)
    return fail(MH_BAD_ARGUMENT,"IsImageGray: null result");
  const uint32_t colour=image->number_channels-(image->alpha_offset >= 0 ? 1u : 0u);
  if (colour < 3)
    {
      *is_gray=1;
      return MH_OK;
    }
  DeviceGuard guard;
  Resident img;
  int device=resolve_device(image);
  MH_TRY(img.open(image,0,image->memory == MH_MEMORY_DEVICE ? (hipStream_t) image->stream :
    library_stream(device),device));
  MH_HIP(guard.enter(img.view.device));
  Temp flag;
  MH_TRY(flag.alloc(img.view.device,sizeof(unsigned int),img.view.stream));
  MH_HIP(hipMemsetAsync(flag.ptr,0,sizeof(unsigned int),img.view.stream));
  MH_TRY(launch_gray_check(img.view,image,flag.as<unsigned int>()));
  unsigned int host=0;
  MH_HIP(hipMemcpyAsync(&host,flag.ptr,sizeof(host),hipMemcpyDeviceToHost,img.view.stream));
  MH_HIP(hipStreamSynchronize(img.view.stream));
  *is_gray=host == 0 ? 1 : 0;
  return MH_OK;
}

// histogram -> LUT -> apply, all on the stream, no host round trip.  `colour_flag` (optional)
// is the gray-scan word: when it says "gray" the LUT builder leaves the mask at zero and the
// apply kernel touches nothing.
static MhStatus histogram_lut_apply(const View &view,const MhImage *image,int mode,bool equalize,
  double black_point,double white_limit,const unsigned int *colour_flag)
{
  const size_t n=(size_t) MH_HISTOGRAM_BINS*(size_t) view.channels;
  Temp hist;
  MH_TRY(hist.alloc(view.device,n*sizeof(unsigned long long),view.stream));
  MH_HIP(hipMemsetAsync(hist.ptr,0,n*sizeof(unsigned long long),view.stream));
  MH_TRY(launch_histogram(view,mode,image,hist.as<unsigned long long>()));
  return apply_histogram_lut(view,image,hist.as<unsigned long long>(),mode,equalize,black_point,
    white_limit,colour_flag);
}

extern "C++" {
namespace mh {
MhStatus equalize_view(const View &view,const MhImage *image)
{
  const int mode=(image->channel_mask & MH_SYNC_CHANNELS) != 0 ? 1 : 0;   // enhance.c:2125-2129
  return histogram_lut_apply(view,image,mode,true,0.0,0.0,nullptr);
}
}
}

// ContrastStretchImage, enhance.c:1544-1818
MH_API MhStatus MagickHipContrastStretchImage(MhImage *image,double black_point,
  double white_point,int *became_gray)
{
  MH_TRY(check_image(image,"ContrastStretchImage"));
  if (became_gray != nullptr)
    *became_gray=0;
  InPlace io;
  MH_TRY(io.open(image));
  const View &view=io.img.view;
  // IdentifyImageType side effect, enhance.c:1586-1588: a colour image whose
  // pixels are all gray is re-laid-out as a GRAY image by the reference; that
  // is the caller's job (SetImageColorspace), so hand such images back untouched.
  // The scan's verdict gates the LUT on the device; the host reads it once, at the end.
  const uint32_t colour=image->number_channels-(image->alpha_offset >= 0 ? 1u : 0u);
  const bool scan=(colour >= 3) && ((image->colorspace == MH_COLORSPACE_SRGB) ||
    (image->colorspace == MH_COLORSPACE_RGB));
  Temp flag;
  if (scan)
    {
      MH_TRY(flag.alloc(view.device,sizeof(unsigned int),view.stream));
      MH_HIP(hipMemsetAsync(flag.ptr,0,sizeof(unsigned int),view.stream));
      MH_TRY(launch_gray_check(view,image,flag.as<unsigned int>()));
    }
  // enhance.c:1637-1643: every channel bins the intensity under the default mask
  const int mode=image->channel_mask == MH_ALL_CHANNELS ? 1 : 0;
  MH_TRY(histogram_lut_apply(view,image,mode,false,black_point,
    (double) image->columns*(double) image->rows-white_point,scan ? flag.as<unsigned int>() : nullptr));
  if (scan)
    {
      unsigned int host=0;
      MH_HIP(hipMemcpyAsync(&host,flag.ptr,sizeof(host),hipMemcpyDeviceToHost,view.stream));
      MH_HIP(hipStreamSynchronize(view.stream));
      if (host == 0)
        {
          if (became_gray != nullptr)
            *became_gray=1;
          return fail(MH_UNSUPPORTED,"ContrastStretchImage: image is gray; convert it to the "
            "GRAY colourspace first (IdentifyImageType, enhance.c:1586)");
        }
    }
  return io.img.commit();
}

// The second half of EqualizeImage / ContrastStretchImage for a caller that holds the histogram
// (the all-reduced table of a row-sharded image): LUT construction and application on the
// device, nothing comes back to the host.
MH_API MhStatus MagickHipApplyHistogram(MhImage *image,const uint64_t *histogram,int intensity_mode,
  int equalize,double black_point,double white_point,size_t image_rows)
{
  MH_TRY(check_image(image,"ApplyHistogram"));
  if (histogram == nullptr)
    return fail(MH_BAD_ARGUMENT,"ApplyHistogram: null histogram");
  InPlace io;
  MH_TRY(io.open(image));
  const View &view=io.img.view;
  const size_t n=(size_t) MH_HISTOGRAM_BINS*(size_t) view.channels;
  Temp table;
  const unsigned long long *device_table=reinterpret_cast<const unsigned long long *>(histogram);
  if (image->memory == MH_MEMORY_HOST)
    {
      MH_TRY(upload_table(table,view.device,view.stream,histogram,n*sizeof(unsigned long long)));
      device_table=table.as<unsigned long long>();
    }
  const double rows=(double) (image_rows == 0 ? image->rows : image_rows);
  MH_TRY(apply_histogram_lut(view,image,device_table,intensity_mode != 0 ? 1 : 0,equalize != 0,black_point,
    (double) image->columns*rows-white_point,nullptr));
  return io.img.commit();
}

// EqualizeImage, enhance.c:2040-2280
MH_API MhStatus MagickHipEqualizeImage(MhImage *image)
{
  MH_TRY(check_image(image,"EqualizeImage"));
  InPlace io;
  MH_TRY(io.open(image));
  const View &view=io.img.view;
  MH_TRY(equalize_view(view,image));
  return io.img.commit();
}

// CLAHEImage, enhance.c:616-785
MH_API MhStatus MagickHipCLAHEImage(MhImage *image,size_t width,size_t height,size_t number_bins,
  double clip_limit)
{
  MH_TRY(check_image(image,"CLAHEImage"));
  const MhColorspace from=(MhColorspace) image->colorspace;
  // the reference re-lays gray frames out as three channels on the way to Lab; four plain channels
  // are no R,G,B[,A]
  const uint32_t colour=image->number_channels-(image->alpha_offset >= 0 ? 1u : 0u);
  if (colour != 3)
    return fail(MH_UNSUPPORTED,"CLAHEImage needs three colour channels");
  if ((from != MH_COLORSPACE_LAB) && !colorspace_is_accelerated(from))
    return fail(MH_UNSUPPORTED,"CLAHEImage: colourspace %d -> Lab is not accelerated",(int) from);
  InPlace io;
  MH_TRY(io.open(image));
  const View &view=io.img.view;
  MH_TRY(clahe_check(view,width,height,number_bins,clip_limit));
  // Both conversions run as the bit-identical ones whatever the call's mode: one level of L across
  // a bin boundary moves a count and with it the mapped value by a whole bin step.  The channel
  // mask plays no part: the reference's transforms store R, G and B past it (colorspace.c), as
  // launch_colorspace does, and so does the write-back of L (enhance.c:761).
  MhImage exact=*image;
  exact.precision=MH_IMAGE_PRECISION(MH_PRECISION_EXACT);
  set_call_precision(&exact);
  if (from != MH_COLORSPACE_LAB)
    MH_TRY(launch_colorspace(view,from,MH_COLORSPACE_LAB,&exact));
  MH_TRY(launch_clahe(view,width,height,number_bins,clip_limit));
  if (from != MH_COLORSPACE_LAB)
    MH_TRY(launch_colorspace(view,MH_COLORSPACE_LAB,from,&exact));
  return io.img.commit();
}

// TransformImageColorspace, colorspace.c:1751-1783
MH_API MhStatus MagickHipTransformImageColorspace(MhImage *image,MhColorspace colorspace)
{
  MH_TRY(check_image(image,"TransformImageColorspace"));
  const MhColorspace from=(MhColorspace) image->colorspace;
  if (from == colorspace)
    return MH_OK;
  if ((colorspace == MH_COLORSPACE_GRAY) || (colorspace == MH_COLORSPACE_LINEARGRAY))
    {
      // sRGB -> GRAY / LinearGRAY (colorspace.c:843-957): gray = 0.212656 R + 0.715158 G +
      // 0.072186 B of the samples (GRAY) or of their gamma-decoded values (LinearGRAY), written
      // into the gray (= first) channel — the expression, operation by operation, of
      // GetPixelIntensity's Rec709Luma / Rec709Luminance on an sRGB image (pixel.c:2219-2235),
      // i.e. GrayscaleImage's kernel.  The channel LAYOUT stays: re-laying the pixels out as one
      // gray channel is SetImageColorspace's part (the caller's, as after GrayscaleImage,
      // enhance.c:2648-2652).
      const uint32_t colours=image->number_channels-(image->alpha_offset >= 0 ? 1u : 0u);
      if ((from != MH_COLORSPACE_SRGB) || (colours != 3))
        return fail(MH_UNSUPPORTED,"colourspace %d -> gray: only from sRGB with three colour channels",(int) from);
      InPlace io;
      MH_TRY(io.open(image));
      MH_TRY(launch_grayscale(io.img.view,colorspace == MH_COLORSPACE_GRAY ? (int) MH_INTENSITY_REC709LUMA :
        (int) MH_INTENSITY_REC709LUMINANCE,image));
      MH_TRY(io.img.commit());
      image->colorspace=(uint32_t) colorspace;
      return MH_OK;
    }
  if (!colorspace_is_accelerated(from) || !colorspace_is_accelerated(colorspace))
    return fail(MH_UNSUPPORTED,"colourspace %d -> %d is not accelerated",(int) from,(int) colorspace);
  const uint32_t colour=image->number_channels-(image->alpha_offset >= 0 ? 1u : 0u);
  if (colour != 3)
    return fail(MH_UNSUPPORTED,"colourspace transform needs three colour channels");
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(launch_colorspace(io.img.view,from,colorspace,image));
  MH_TRY(io.img.commit());
  image->colorspace=(uint32_t) colorspace;
  return MH_OK;
}

// TransformImageColorspace followed by ContrastStretchImage, as one call.  The results are those
// of the two calls; what the pair can share is the pass over the pixels: FAST sRGB -> Lab on
// RGBA Q16 converts and bins the intensity of what it stores in the same kernel (histogram.hip,
// lab_histogram_fast_kernel).  MagickHipBatchImages uses it for adjacent operators of a chain.
MH_API MhStatus MagickHipTransformColorspaceContrastStretchImage(MhImage *image,MhColorspace colorspace,
  double black_point,double white_point)
{
  MH_TRY(check_image(image,"TransformColorspaceContrastStretchImage"));
  const uint32_t colour=image->number_channels-(image->alpha_offset >= 0 ? 1u : 0u);
  if (((MhColorspace) image->colorspace == MH_COLORSPACE_SRGB) && (colorspace == MH_COLORSPACE_LAB) &&
      (colour == 3) && (image->channel_mask == MH_ALL_CHANNELS) && (image->memory == MH_MEMORY_DEVICE))
    {
      InPlace io;
      MH_TRY(io.open(image));
      const View &view=io.img.view;
      MhImage lab=*image;
      lab.colorspace=(uint32_t) MH_COLORSPACE_LAB;
      bool fused=false;
      {
        // three launches: convert + bin, levels, map (histogram.hip)
        uint32_t update=0;
        for (uint32_t c=0; c < image->number_channels; c++)
          if ((image->channel_traits[c] & MH_TRAIT_UPDATE) != 0)
            update|=1u<<c;
        MH_TRY(launch_lab_fast_contrast_stretch(view,&lab,black_point,
          (double) image->columns*(double) image->rows-white_point,update,&fused));
        if (fused)
          {
            image->colorspace=(uint32_t) MH_COLORSPACE_LAB;
            return io.img.commit();
          }
      }
      const size_t n=(size_t) MH_HISTOGRAM_BINS*(size_t) view.channels;
      Temp hist;
      MH_TRY(hist.alloc(view.device,n*sizeof(unsigned long long),view.stream));
      MH_HIP(hipMemsetAsync(hist.ptr,0,n*sizeof(unsigned long long),view.stream));
      MH_TRY(launch_lab_fast_with_histogram(view,&lab,hist.as<unsigned long long>(),&fused));
      if (fused)
        {
          image->colorspace=(uint32_t) MH_COLORSPACE_LAB;
          MH_TRY(apply_histogram_lut(view,image,hist.as<unsigned long long>(),1,false,black_point,
            (double) image->columns*(double) image->rows-white_point,nullptr));
          return io.img.commit();
        }
    }
  MH_TRY(MagickHipTransformImageColorspace(image,colorspace));
  return MagickHipContrastStretchImage(image,black_point,white_point,nullptr);
}

// ContrastImage, enhance.c:1392-1480
MH_API MhStatus MagickHipContrastImage(MhImage *image,int sharpen)
{
  MH_TRY(check_image(image,"ContrastImage"));
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(launch_contrast(io.img.view,sharpen != 0));
  return io.img.commit();
}

// ModulateImage, enhance.c:3665-3900 (HSL and HSB models)
MH_API MhStatus MagickHipModulateImage(MhImage *image,double percent_brightness,
  double percent_saturation,double percent_hue,int colorspace)
{
  MH_TRY(check_image(image,"ModulateImage"));
  bool generic=false;
  switch (colorspace)
  {
    case MH_COLORSPACE_UNDEFINED: case MH_COLORSPACE_HSL: case MH_COLORSPACE_HSB:
      break;
    case MH_COLORSPACE_HCL: case MH_COLORSPACE_HCLP: case MH_COLORSPACE_HSI: case MH_COLORSPACE_HSV:
    case MH_COLORSPACE_HWB: case MH_COLORSPACE_LCH: case MH_COLORSPACE_LCHAB: case MH_COLORSPACE_LCHUV:
      generic=true;                               // enhance.c:3826-3890
      break;
    default:
      // (any other value falls into ModulateHSL's `default:` in the reference; the shim maps
      // those to HSL before calling)
      return fail(MH_UNSUPPORTED,"ModulateImage: colour model %d is not accelerated",colorspace);
  }
  InPlace io;
  MH_TRY(io.open(image));
  // the loop invariants of the Modulate* helpers, enhance.c:3462-3632
  const double hue_shift=fmod((percent_hue-100.0),200.0)/200.0;
  const double saturation_scale=0.01*percent_saturation;
  const double brightness_scale=0.01*percent_brightness;
  if (generic)
    MH_TRY(launch_modulate_generic(io.img.view,(MhColorspace) colorspace,hue_shift,saturation_scale,
      brightness_scale));
  else
    MH_TRY(launch_modulate(io.img.view,colorspace == MH_COLORSPACE_HSB,hue_shift,saturation_scale,
      brightness_scale));
  return io.img.commit();
}

// ImportImagePixels / ExportImagePixels, pixel.c:4164 / :1962
static MhStatus pixel_io(bool import,const MhImage *image,ptrdiff_t x,ptrdiff_t y,size_t width,
  size_t height,const char *map,MhStorageType type,void *pixels,MhMemoryKind pixels_memory)
{
  const char *what=import ? "ImportImagePixels" : "ExportImagePixels";
  MH_TRY(check_image(image,what));
  if ((map == nullptr) || (pixels == nullptr))
    return fail(MH_BAD_ARGUMENT,"%s: null map or pixels",what);
  if ((width == 0) || (height == 0) || (x < 0) || (y < 0) ||
      ((size_t) x+width > image->columns) || ((size_t) y+height > image->rows))
    return fail(MH_UNSUPPORTED,"%s: the region must lie inside the image",what);
  const size_t element=storage_size(type,(MhQuantumKind) image->quantum);
  if (element == 0)
    return fail(MH_BAD_ARGUMENT,"%s: unknown storage type %d",what,(int) type);
  const size_t bytes=width*height*strlen(map)*element;
  DeviceGuard guard;
  Resident img;
  int device=resolve_device(image);
  hipStream_t stream=image->memory == MH_MEMORY_DEVICE ? (hipStream_t) image->stream :
    library_stream(device);
  // import modifies the image (upload + download unless the map covers it: keep it simple,
  // mode 2); export only reads it
  MH_TRY(img.open(image,import ? 2 : 0,stream,device));
  img.view.stream=stream;
  img.view.device=device;
  MH_HIP(guard.enter(device));
  Temp staged;
  void *buffer=pixels;
  if (pixels_memory == MH_MEMORY_HOST)
    {
      MH_TRY(staged.alloc(device,bytes,stream));
      buffer=staged.ptr;
      if (import)
        MH_HIP(hipMemcpyAsync(buffer,pixels,bytes,hipMemcpyHostToDevice,stream));
      else
        {
          // pads the reference leaves untouched must survive the round trip
          bool has_pad=false;
          for (const char *m=map; *m != 0; m++)
            has_pad|=(*m == 'P') || (*m == 'p');
          if (has_pad)
            MH_HIP(hipMemcpyAsync(buffer,pixels,bytes,hipMemcpyHostToDevice,stream));
        }
    }
  MH_TRY(launch_pixel_io(import,img.view,image,(int) x,(int) y,(int) width,(int) height,map,type,
    buffer));
  if (!import && (pixels_memory == MH_MEMORY_HOST))
    {
      MH_HIP(hipMemcpyAsync(pixels,buffer,bytes,hipMemcpyDeviceToHost,stream));
      MH_HIP(hipStreamSynchronize(stream));
    }
  return img.commit();
}

MH_API MhStatus MagickHipImportImagePixels(MhImage *image,ptrdiff_t x,ptrdiff_t y,size_t width,
  size_t height,const char *map,MhStorageType type,const void *pixels,MhMemoryKind pixels_memory)
{
  return pixel_io(true,image,x,y,width,height,map,type,const_cast<void *>(pixels),pixels_memory);
}

MH_API MhStatus MagickHipExportImagePixels(const MhImage *image,ptrdiff_t x,ptrdiff_t y,
  size_t width,size_t height,const char *map,MhStorageType type,void *pixels,
  MhMemoryKind pixels_memory)
{
  return pixel_io(false,image,x,y,width,height,map,type,pixels,pixels_memory);
}

// GrayscaleImage, enhance.c:2476-2660
MH_API MhStatus MagickHipGrayscaleImage(MhImage *image,MhIntensityMethod method)
{
  MH_TRY(check_image(image,"GrayscaleImage"));
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(launch_grayscale(io.img.view,(int) method,image));
  return io.img.commit();
}

// FunctionImage, statistic.c:1069-1160
MH_API MhStatus MagickHipFunctionImage(MhImage *image,MhFunction function,
  size_t number_parameters,const double *parameters)
{
  MH_TRY(check_image(image,"FunctionImage"));
  if ((number_parameters != 0) && (parameters == nullptr))
    return fail(MH_BAD_ARGUMENT,"FunctionImage: null parameters");
  if ((function < MH_FUNCTION_ARCSIN) || (function > MH_FUNCTION_SINUSOID))
    return fail(MH_BAD_ARGUMENT,"FunctionImage: unknown function %d",(int) function);
  uint32_t update=0;
  for (uint32_t c=0; c < image->number_channels; c++)
    if ((image->channel_traits[c] & MH_TRAIT_UPDATE) != 0)
      update|=1u<<c;
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(launch_function(io.img.view,(int) function,number_parameters,parameters,update));
  return io.img.commit();
}

// ------------------------------------------------------------------ threshold.c
// The frames the reference's IsGrayColorspace() holds for gray: fewer than three colour channels
// are laid out that way whatever the descriptor's colourspace says (pixel_intensity.hpp).
static bool threshold_gray_frame(const MhImage *image)
{
  const uint32_t colours=image->number_channels-(image->alpha_offset >= 0 ? 1u : 0u);
  return (image->colorspace == MH_COLORSPACE_GRAY) || (image->colorspace == MH_COLORSPACE_LINEARGRAY) ||
    (colours < 3);
}

// KapurThreshold, threshold.c:392-489
static double kapur_threshold(const double *histogram)
{
  double black_entropy[256],cumulative_histogram[256],white_entropy[256];
  cumulative_histogram[0]=histogram[0];
  for (int i=1; i <= 255; i++)
    cumulative_histogram[i]=cumulative_histogram[i-1]+histogram[i];
  const double epsilon=2.22507385850720140E-308;      // MagickMinimumValue, magick-type.h:116
  for (int j=0; j <= 255; j++)
    {
      black_entropy[j]=0.0;
      if (cumulative_histogram[j] > epsilon)
        {
          double entropy=0.0;
          for (int i=0; i <= j; i++)
            if (histogram[i] > epsilon)
              entropy-=histogram[i]/cumulative_histogram[j]*log(histogram[i]/cumulative_histogram[j]);
          black_entropy[j]=entropy;
        }
      white_entropy[j]=0.0;
      if ((1.0-cumulative_histogram[j]) > epsilon)
        {
          double entropy=0.0;
          for (int i=j+1; i <= 255; i++)
            if (histogram[i] > epsilon)
              entropy-=histogram[i]/(1.0-cumulative_histogram[j])*log(histogram[i]/(1.0-cumulative_histogram[j]));
          white_entropy[j]=entropy;
        }
    }
  double maximum_entropy=black_entropy[0]+white_entropy[0];
  size_t threshold=0;
  for (int j=1; j <= 255; j++)
    if ((black_entropy[j]+white_entropy[j]) > maximum_entropy)
      {
        maximum_entropy=black_entropy[j]+white_entropy[j];
        threshold=(size_t) j;
      }
  return 100.0*threshold/255;
}

// OTSUThreshold, threshold.c:491-568
static double otsu_threshold(const double *histogram)
{
  double myu[256],omega[256],probability[256],sigma[256];
  for (int i=0; i <= 255; i++)
    probability[i]=histogram[i];
  omega[0]=probability[0];
  myu[0]=0.0;
  for (int i=1; i <= 255; i++)
    {
      omega[i]=omega[i-1]+probability[i];
      myu[i]=myu[i-1]+i*probability[i];
    }
  double threshold=0,max_sigma=0.0;
  for (int i=0; i < 255; i++)
    {
      sigma[i]=0.0;
      if ((omega[i] != 0.0) && (omega[i] != 1.0))
        sigma[i]=pow(myu[255]*omega[i]-myu[i],2.0)/(omega[i]*(1.0-omega[i]));
      if (sigma[i] > max_sigma)
        {
          max_sigma=sigma[i];
          threshold=(double) i;
        }
    }
  return 100.0*threshold/255;
}

// TriangleThreshold, threshold.c:570-658
static double triangle_threshold(const double *histogram)
{
  ssize_t start=0,end=0,max=0,threshold=0;
  for (ssize_t i=0; i <= 255; i++)
    if (histogram[i] > 0.0)
      {
        start=i;
        break;
      }
  for (ssize_t i=255; i >= 0; i--)
    if (histogram[i] > 0.0)
      {
        end=i;
        break;
      }
  double count=0.0;
  for (ssize_t i=0; i <= 255; i++)
    if (histogram[i] > count)
      {
        max=i;
        count=histogram[i];
      }
  const double x1=(double) max,y1=histogram[max];
  double x2=(double) end;
  if ((max-start) >= (end-max))
    x2=(double) start;
  const double y2=0.0;
  const double a=y1-y2,b=x2-x1;
  const double c=(-1.0)*(a*x1+b*y1);
  const double inverse_ratio=1.0/sqrt(a*a+b*b+c*c);
  double max_distance=0.0;
  if (x2 == (double) start)
    for (ssize_t i=start; i < max; i++)
      {
        const double segment=inverse_ratio*(a*i+b*histogram[i]+c);
        const double distance=sqrt(segment*segment);
        if ((distance > max_distance) && (segment > 0.0))
          {
            threshold=i;
            max_distance=distance;
          }
      }
  else
    for (ssize_t i=end; i > max; i--)
      {
        const double segment=inverse_ratio*(a*i+b*histogram[i]+c);
        const double distance=sqrt(segment*segment);
        if ((distance > max_distance) && (segment < 0.0))
          {
            threshold=i;
            max_distance=distance;
          }
      }
  return 100.0*threshold/255;
}

// AutoThresholdImage's normalisation and selection, threshold.c:718-748, on the host
MH_API MhStatus MhAutoThresholdFromHistogram(const double counts[256],MhAutoThresholdMethod method,
  double *threshold_percent)
{
  if ((counts == nullptr) || (threshold_percent == nullptr))
    return fail(MH_BAD_ARGUMENT,"AutoThresholdFromHistogram: null argument");
  double histogram[256],sum=0.0;
  for (int i=0; i <= 255; i++)
    sum+=counts[i];
  const double gamma=perceptible_reciprocal(sum);
  for (int i=0; i <= 255; i++)
    histogram[i]=gamma*counts[i];
  switch (method)
  {
    case MH_AUTO_THRESHOLD_KAPUR: *threshold_percent=kapur_threshold(histogram); break;
    case MH_AUTO_THRESHOLD_TRIANGLE: *threshold_percent=triangle_threshold(histogram); break;
    case MH_AUTO_THRESHOLD_OTSU: default: *threshold_percent=otsu_threshold(histogram); break;
  }
  return MH_OK;
}

// BilevelImage on an open frame: threshold.c:828-829 retags a frame outside the gray colourspaces
// as sRGB before the intensity is formed
static MhStatus bilevel_view(const View &view,MhImage *image,double threshold)
{
  if (!threshold_gray_frame(image))
    image->colorspace=MH_COLORSPACE_SRGB;
  return launch_bilevel(view,threshold,image);
}

MH_API MhStatus MagickHipBilevelImage(MhImage *image,double threshold)
{
  MH_TRY(check_image(image,"BilevelImage"));
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(bilevel_view(io.img.view,image,threshold));
  return io.img.commit();
}

MH_API MhStatus MagickHipAutoThresholdImage(MhImage *image,MhAutoThresholdMethod method,double *threshold_percent)
{
  MH_TRY(check_image(image,"AutoThresholdImage"));
  InPlace io;
  MH_TRY(io.open(image));
  const View &view=io.img.view;
  Temp table;
  MH_TRY(table.alloc(view.device,256*sizeof(unsigned long long),view.stream));
  MH_TRY(launch_threshold_histogram(view,image,table.as<unsigned long long>()));
  unsigned long long host[256];
  MH_HIP(hipMemcpyAsync(host,table.ptr,sizeof(host),hipMemcpyDeviceToHost,view.stream));
  MH_HIP(hipStreamSynchronize(view.stream));
  double counts[256],percent=0.0;
  for (int i=0; i < 256; i++)
    counts[i]=(double) host[i];          // the reference counts in doubles: exact below 2^53
  MH_TRY(MhAutoThresholdFromHistogram(counts,method,&percent));
  if (threshold_percent != nullptr)
    *threshold_percent=percent;
  MH_TRY(bilevel_view(view,image,kQuantumRange*percent/100.0));
  return io.img.commit();
}

// Black / White / RangeThresholdImage re-lay a gray frame out as sRGB (threshold.c:961, :2401, :2552)
static MhStatus threshold_colour_frame(const MhImage *image,const char *what)
{
  MH_TRY(check_image(image,what));
  if (threshold_gray_frame(image))
    return fail(MH_UNSUPPORTED,"%s: the reference re-lays a gray frame out as sRGB",what);
  return MH_OK;
}

MH_API MhStatus MagickHipBlackThresholdImage(MhImage *image,const double thresholds[MH_MAX_CHANNELS])
{
  MH_TRY(threshold_colour_frame(image,"BlackThresholdImage"));
  if (thresholds == nullptr)
    return fail(MH_BAD_ARGUMENT,"BlackThresholdImage: null thresholds");
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(launch_black_white_threshold(io.img.view,false,thresholds,image));
  return io.img.commit();
}

MH_API MhStatus MagickHipWhiteThresholdImage(MhImage *image,const double thresholds[MH_MAX_CHANNELS])
{
  MH_TRY(threshold_colour_frame(image,"WhiteThresholdImage"));
  if (thresholds == nullptr)
    return fail(MH_BAD_ARGUMENT,"WhiteThresholdImage: null thresholds");
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(launch_black_white_threshold(io.img.view,true,thresholds,image));
  return io.img.commit();
}

MH_API MhStatus MagickHipRangeThresholdImage(MhImage *image,double low_black,double low_white,double high_white,
  double high_black)
{
  MH_TRY(threshold_colour_frame(image,"RangeThresholdImage"));
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(launch_range_threshold(io.img.view,low_black,low_white,high_white,high_black,
    kQuantumRange*perceptible_reciprocal(low_white-low_black),
    kQuantumRange*perceptible_reciprocal(high_black-high_white),image));
  return io.img.commit();
}

// ------------------------------------------------------------------ the level operators
MH_API MhStatus MagickHipLevelImage(MhImage *image,double black_point,double white_point,double gamma)
{
  MH_TRY(check_image(image,"LevelImage"));
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(level_view(io.img.view,update_mask_of(image),black_point,white_point,gamma));
  return io.img.commit();
}

MH_API MhStatus MagickHipLevelizeImage(MhImage *image,double black_point,double white_point,double gamma)
{
  MH_TRY(check_image(image,"LevelizeImage"));
  InPlace io;
  MH_TRY(io.open(image));
  const View &view=io.img.view;
  const uint32_t update=update_mask_of(image);
  if ((gamma != 1.0) && (view.quantum == MH_QUANTUM_U16))
    {
      const double p[4]={white_point-black_point,black_point,gamma,0.0};
      MH_TRY(apply_levels_table(view,LEVELS_TABLE_LEVELIZE,p,update,"levels_levelize_table"));
    }
  else
    {
      LevelsParams params;
      params.mode=gamma != 1.0 ? MH_LEVELS_LEVELIZE_POW : MH_LEVELS_LEVELIZE;     // pow(v,1.0) is v
      params.update_mask=update;
      params.a=white_point-black_point;
      params.b=black_point;
      params.c=gamma;
      MH_TRY(launch_levels_point(view,params));
    }
  return io.img.commit();
}

// GammaImage's map, enhance.c:2354-2362
MH_API MhStatus MhGammaLUT(double gamma,MhQuantumKind quantum,double *lut)
{
  if (lut == nullptr)
    return fail(MH_BAD_ARGUMENT,"GammaLUT: null LUT");
  memset(lut,0,(size_t) MH_HISTOGRAM_BINS*sizeof(double));
  if (gamma != 0.0)
    for (size_t i=0; i <= MH_MAXMAP; i++)
      lut[i]=scale_map_to_quantum((double) MH_MAXMAP*pow((double) i/(double) MH_MAXMAP,perceptible_reciprocal(gamma)),
        quantum);
  return MH_OK;
}

MH_API MhStatus MagickHipGammaImage(MhImage *image,double gamma)
{
  MH_TRY(check_image(image,"GammaImage"));
  if (gamma == 1.0)
    return MH_OK;
  InPlace io;
  MH_TRY(io.open(image));
  const double p[4]={gamma,0.0,0.0,0.0};
  MH_TRY(apply_levels_table(io.img.view,LEVELS_TABLE_GAMMA,p,update_mask_of(image),"levels_gamma_table"));
  return io.img.commit();
}

MH_API MhStatus MagickHipNegateImage(MhImage *image,int grayscale)
{
  MH_TRY(check_image(image,"NegateImage"));
  InPlace io;
  MH_TRY(io.open(image));
  LevelsParams params;
  params.mode=grayscale != 0 ? MH_LEVELS_NEGATE_GRAY : MH_LEVELS_NEGATE;
  params.update_mask=update_mask_of(image);
  params.colours=(int) image->number_channels-(image->alpha_offset >= 0 ? 1 : 0);
  MH_TRY(launch_levels_point(io.img.view,params));
  return io.img.commit();
}

// The magnitude below which a float sample is doubtful under a sigmoidal (mh_internal.hpp, LevelsDoubt).  Around a
// sample of 0 the result r is r'(0)*q, and the libm's last bits are worth E = QuantumRange*2^-53/|sig1-sig0| of it
// (sharpen) or QuantumRange*2^-53*|b| (inverse: b+a*atanh(...) with a*atanh(...) = -b at the zero).  A result is kept
// from the device from 2^30*E on, where E is 2^-6 of a float's last place: |q| >= 2*2^30*E/|r'(0)|, the 2 for the
// curvature.  r'(0) = a*(1-sig0^2)/(sig1-sig0) (sharpen), a*(sig1-sig0)/(1-sig0^2) (inverse); where the curve is
// saturated at 0 (1-sig0^2 below 1e-4) the slope says nothing and every sample is the host's.
static double sigmoidal_doubt(bool sharpen,const double *p)
{
  const double slack=1.0-p[2]*p[2],span=fabs(p[3]-p[2]);
  if (!(slack > 1.0e-4) || !(span > 0.0))
    return HUGE_VAL;
  const double last=ldexp(kQuantumRange,-23);             // 2^30 * QuantumRange * 2^-53
  if (sharpen)
    return 2.0*(last/span)/(p[0]*slack/span);
  return 2.0*(last*(fabs(p[1])+1.0e-3))/(p[0]*span/slack);
}

// A sigmoidal on a float frame: the point kernel, and the doubtful samples from the host's libm
static MhStatus sigmoidal_float(const View &view,LevelsParams params,int curve,const double *p)
{
  if ((view.columns == 0) || (view.rows == 0) || (params.update_mask == 0))
    return MH_OK;
  params.doubt=sigmoidal_doubt(curve == LEVELS_TABLE_SIGMOIDAL,p);
  Temp counters;
  MH_TRY(counters.alloc(view.device,2*sizeof(unsigned long long),view.stream));
  MH_HIP(hipMemsetAsync(counters.ptr,0,2*sizeof(unsigned long long),view.stream));
  MH_TRY(launch_levels_doubt_count(view,params,counters.as<unsigned long long>()));
  unsigned long long count=0;
  MH_HIP(hipMemcpyAsync(&count,counters.ptr,sizeof(count),hipMemcpyDeviceToHost,view.stream));
  MH_HIP(hipStreamSynchronize(view.stream));
  if (count == 0)
    return launch_levels_point(view,params);
  Temp list;
  MH_TRY(list.alloc(view.device,(size_t) count*sizeof(LevelsDoubt),view.stream));
  params.doubt_list=list.as<LevelsDoubt>();
  params.doubt_count=counters.as<unsigned long long>()+1;
  params.doubt_capacity=count;
  MH_TRY(launch_levels_point(view,params));
  std::vector<LevelsDoubt> host((size_t) count);
  unsigned long long recorded=0;
  MH_HIP(hipMemcpyAsync(&recorded,counters.as<unsigned long long>()+1,sizeof(recorded),hipMemcpyDeviceToHost,view.stream));
  MH_HIP(hipMemcpyAsync(host.data(),list.ptr,host.size()*sizeof(LevelsDoubt),hipMemcpyDeviceToHost,view.stream));
  MH_HIP(hipStreamSynchronize(view.stream));
  if (recorded != count)
    return fail(MH_DEVICE_ERROR,"SigmoidalContrastImage: %llu doubtful samples counted, %llu recorded",count,recorded);
  for (size_t k=0; k < host.size(); k++)
    host[k].value=(float) clamp_to_quantum(levels_curve(curve,p,(double) host[k].original),MH_QUANTUM_F32);
  MH_HIP(hipMemcpyAsync(list.ptr,host.data(),host.size()*sizeof(LevelsDoubt),hipMemcpyHostToDevice,view.stream));
  MH_TRY(launch_levels_scatter(view,list.as<LevelsDoubt>(),count));
  MH_HIP(hipStreamSynchronize(view.stream));             // `host` leaves with this call
  return MH_OK;
}

MH_API MhStatus MagickHipSigmoidalContrastImage(MhImage *image,int sharpen,double contrast,double midpoint)
{
  MH_TRY(check_image(image,"SigmoidalContrastImage"));
  if (contrast < kMagickEpsilon)
    return MH_OK;
  InPlace io;
  MH_TRY(io.open(image));
  const View &view=io.img.view;
  const uint32_t update=update_mask_of(image);
  // Sigmoidal(a,b,x) = tanh((0.5*a)*(x-b)), enhance.c:4207; the two constants of the call from the host's tanh
  const double b=kQuantumScale*midpoint;
  const double sig0=tanh((0.5*contrast)*(0.0-b)),sig1=tanh((0.5*contrast)*(1.0-b));
  const double p[4]={sharpen != 0 ? 0.5*contrast : 2.0/contrast,b,sig0,sig1};
  if (view.quantum == MH_QUANTUM_U16)
    MH_TRY(apply_levels_table(view,sharpen != 0 ? LEVELS_TABLE_SIGMOIDAL : LEVELS_TABLE_SIGMOIDAL_INVERSE,p,update,
      "levels_sigmoidal_table"));
  else
    {
      LevelsParams params;
      params.mode=sharpen != 0 ? MH_LEVELS_SIGMOIDAL : MH_LEVELS_SIGMOIDAL_INVERSE;
      params.update_mask=update;
      params.a=p[0];
      params.b=p[1];
      params.c=p[2];
      params.d=p[3];
      const double clamped=sig0 < -1+kMagickEpsilon ? -1+kMagickEpsilon : (sig0 > 1-kMagickEpsilon ? 1-kMagickEpsilon : sig0);
      params.e=atanh(clamped);
      MH_TRY(sigmoidal_float(view,params,sharpen != 0 ? LEVELS_TABLE_SIGMOIDAL : LEVELS_TABLE_SIGMOIDAL_INVERSE,p));
    }
  return io.img.commit();
}

MH_API MhStatus MagickHipImageRange(const MhImage *image,double *minimum,double *maximum)
{
  MH_TRY(check_image(image,"ImageRange"));
  if ((minimum == nullptr) || (maximum == nullptr))
    return fail(MH_BAD_ARGUMENT,"ImageRange: null result");
  DeviceGuard guard;
  Resident img;
  const int device=resolve_device(image);
  MH_TRY(img.open(image,0,image->memory == MH_MEMORY_DEVICE ? (hipStream_t) image->stream :
    library_stream(device),device));
  MH_HIP(guard.enter(img.view.device));
  double slots[2*(MH_MAX_CHANNELS+1)];
  MH_TRY(range_to_host(img.view,false,slots));
  combine_range(slots,img.view,update_mask_of(image),minimum,maximum);
  return MH_OK;
}

MH_API MhStatus MagickHipMinMaxStretchImage(MhImage *image,double black,double white,double gamma)
{
  MH_TRY(check_image(image,"MinMaxStretchImage"));
  InPlace io;
  MH_TRY(io.open(image));
  MH_TRY(min_max_stretch_view(io.img.view,image,black,white,gamma));
  return io.img.commit();
}

// enhance.c:187-191
MH_API MhStatus MagickHipAutoLevelImage(MhImage *image)
{
  return MagickHipMinMaxStretchImage(image,0.0,0.0,1.0);
}

MH_API MhStatus MagickHipLinearStretchImage(MhImage *image,double black_point,double white_point,size_t *black,
  size_t *white)
{
  MH_TRY(check_image(image,"LinearStretchImage"));
  InPlace io;
  MH_TRY(io.open(image));
  const View &view=io.img.view;
  // enhance.c:3382-3401: counts of ScaleQuantumToMap(ClampToQuantum(intensity)); the intensity
  // histogram gives every channel's column the same counts
  std::vector<unsigned long long> counts;
  MH_TRY(histogram_to_host(view,1,image,counts));
  const size_t C=(size_t) view.channels;
  // enhance.c:3406-3419
  double intensity=0.0;
  ptrdiff_t low,high;
  for (low=0; low < (ptrdiff_t) MH_MAXMAP; low++)
    {
      intensity+=(double) counts[C*(size_t) low];
      if (intensity >= black_point)
        break;
    }
  intensity=0.0;
  for (high=(ptrdiff_t) MH_MAXMAP; high != 0; high--)
    {
      intensity+=(double) counts[C*(size_t) high];
      if (intensity >= white_point)
        break;
    }
  if (black != nullptr)
    *black=(size_t) low;
  if (white != nullptr)
    *white=(size_t) high;
  MH_TRY(level_view(view,update_mask_of(image),scale_map_to_quantum((double) low,view.quantum),
    scale_map_to_quantum((double) high,view.quantum),1.0));
  return io.img.commit();
}

// enhance.c:4130-4140
MH_API MhStatus MagickHipNormalizeImage(MhImage *image)
{
  if (image == nullptr)
    return fail(MH_BAD_ARGUMENT,"NormalizeImage: null image");
  const double black_point=0.02*(double) image->columns*(double) image->rows;
  const double white_point=0.99*(double) image->columns*(double) image->rows;
  return MagickHipContrastStretchImage(image,black_point,white_point,nullptr);
}

// enhance.c:224-252
MH_API MhStatus MagickHipBrightnessContrastImage(MhImage *image,double brightness,double contrast)
{
  double slope=100.0*perceptible_reciprocal(100.0-contrast);
  if (contrast < 0.0)
    slope=0.01*contrast+1.0;
  const double intercept=(0.01*brightness-0.5)*slope+0.5;
  const double coefficients[2]={slope,intercept};
  return MagickHipFunctionImage(image,MH_FUNCTION_POLYNOMIAL,2,coefficients);
}

// tables built since the process started (tests: a second call with the same parameters builds none)
MH_API unsigned long long MhLevelsTablesBuilt(void)
{
  std::lock_guard<std::mutex> guard(levels_tables_lock());
  return levels_tables_built;
}

} // extern "C"
