// The tables and the launch geometry of ResizeImage's two separate passes (imagemagick_amd/csrc/resize_pass_plan.hpp)
// against the contribution lists they are made from: the vertical kernel's dense per-tile weights and row masks, the
// horizontal kernel's per-tile spans, and which of the seven horizontal kernels runs with how many rows in how much LDS.
// The geometries are those of tests/resize_cases.py (TAP_CASES, WIDE_POINT, DEGENERATE_COLUMNS), sizes that are no
// multiple of a tile, and a list with empty windows.  Test infrastructure: built and run by
// tests/test_resize_pass_plan.py (no GPU).
//   g++ -O2 -std=c++17 -I imagemagick_amd/csrc tests/cpu/resize_pass_plan_test.cpp -o /tmp/pass_plan_test
#include "resize_pass_plan.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

struct Table
{
  int out_size=0,max_taps=0;
  std::vector<int> start,count;
  std::vector<double> weight;     // [tap][out]
};

// contribution lists with the windows of resize.c:3364-3380, :3418-3443 (tests/resize_cases.py, windows()); the
// weights are a raised cosine over the window, normalised: positive, all different
static void build(Table &t,int in,int out,double filter_support)
{
  const double epsilon=1.0e-12;
  const double factor=(double) out*(1.0/(double) in);
  const double scale=std::max(1.0/factor+epsilon,1.0);
  const double support=std::max(scale*filter_support,0.5);
  t.out_size=out;
  t.start.assign(out,0); t.count.assign(out,0);
  std::vector<std::vector<double>> w(out);
  t.max_taps=0;
  for (int x=0; x < out; x++)
    {
      const double bisect=(x+0.5)/factor+epsilon;
      const int start=(int) std::max(bisect-support+0.5,0.0);
      const int stop=(int) std::min(bisect+support+0.5,(double) in);
      double density=0.0;
      for (int n=0; n < stop-start; n++)
        {
          const double v=1.05+std::cos(M_PI*((start+n)-bisect+0.5)/(support+1.0));
          w[x].push_back(v);
          density+=v;
        }
      for (double &v : w[x])
        v/=density;
      t.start[x]=start;
      t.count[x]=std::max(stop-start,0);
      t.max_taps=std::max(t.max_taps,t.count[x]);
    }
  t.weight.assign((size_t) t.max_taps*out,0.0);
  for (int x=0; x < out; x++)
    for (int j=0; j < t.count[x]; j++)
      t.weight[(size_t) j*out+x]=w[x][j];
}

static int failures=0;
#define CHECK(cond) do { if (!(cond)) { if (failures < 20) std::printf("FAIL %s line %d: %s\n",g_name,__LINE__,#cond); failures++; } } while (0)
static const char *g_name="";

// tests/resize_cases.py, tap_class(): the kernel's tap count for the class (0: any number)
static int class_taps(int taps)
{
  const int limits[6]={4,6,7,8,16,32};
  for (int limit : limits)
    if (taps <= limit)
      return limit;
  return 0;
}

static void check_vertical(const Table &t)
{
  constexpr int RY=mh::kVerticalRows;
  mh::VerticalPassPlan p;
  mh::build_vertical_pass_plan(p,t);
  const int tiles=(t.out_size+RY-1)/RY;
  CHECK(p.tiles == tiles);
  CHECK((int) p.lo.size() == tiles && (int) p.rows.size() == tiles);
  CHECK(p.w.size() == (size_t) tiles*p.kmax*RY && p.wq.size() == p.w.size() && p.mask.size() == (size_t) tiles*p.kmax);
  int widest=1;
  for (int tile=0; tile < tiles; tile++)
    {
      widest=std::max(widest,p.rows[tile]);
      CHECK(p.rows[tile] <= p.kmax);
      for (int k=0; k < p.kmax; k++)
        {
          const int row=p.lo[tile]+k;
          for (int r=0; r < RY; r++)
            {
              const int y=tile*RY+r;
              const bool inside=(y < t.out_size) && (t.count[y] > 0) && (row >= t.start[y]) && (row < t.start[y]+t.count[y]);
              // every window lies inside the tile's rows
              if ((y < t.out_size) && (t.count[y] > 0))
                CHECK((t.start[y] >= p.lo[tile]) && (t.start[y]+t.count[y] <= p.lo[tile]+p.rows[tile]));
              const double want=inside ? t.weight[(size_t) (row-t.start[y])*t.out_size+y] : 0.0;
              const size_t at=((size_t) tile*p.kmax+k)*RY+r;
              CHECK(p.w[at] == want);
              CHECK(p.wq[at] == want*mh::kPassQuantumScale);
              CHECK(((p.mask[(size_t) tile*p.kmax+k] >> r) & 1u) == (inside ? 1u : 0u));
            }
          CHECK((p.mask[(size_t) tile*p.kmax+k] >> RY) == 0u);
        }
    }
  CHECK(p.kmax == widest);                     // the widest tile
}

static void check_horizontal(const Table &t,int expect_taps)
{
  constexpr int TILE=mh::kHorizontalTile;
  mh::HorizontalPassPlan p;
  mh::build_horizontal_pass_plan(p,t);
  const int tiles=(t.out_size+TILE-1)/TILE;
  CHECK(t.max_taps == expect_taps);
  CHECK((int) p.tile_lo.size() == tiles && (int) p.tile_span.size() == 2*tiles);
  CHECK(p.wq.size() == t.weight.size());
  for (size_t i=0; i < std::min(p.wq.size(),t.weight.size()); i++)
    CHECK(p.wq[i] == t.weight[i]*mh::kPassQuantumScale);
  CHECK(p.maxt == (t.max_taps <= 8 ? class_taps(t.max_taps) : 8));
  int widest=1,reach=0;
  for (int tile=0; tile < tiles; tile++)
    {
      const int lo=p.tile_lo[tile],span=p.tile_span[tile];
      int largest=0;
      widest=std::max(widest,span);
      for (int x=tile*TILE; x < std::min(t.out_size,(tile+1)*TILE); x++)
        {
          CHECK(lo <= t.start[x]);
          CHECK(t.start[x]+t.count[x] <= lo+span);
          CHECK(t.start[x]+p.maxt <= lo+span+p.overhang);
          reach=std::max(reach,t.start[x]+p.maxt-(lo+span));
          largest=std::max(largest,t.count[x]);
        }
      CHECK(p.tile_span[tiles+tile] == largest);       // second half: the tile's largest count
    }
  CHECK(p.max_span == widest);
  CHECK(p.overhang == std::max(reach,0));             // no wider than the farthest read

  // launch geometry, every layout
  for (int channels=1; channels <= 4; channels++)
    for (size_t quantum_bytes : {sizeof(unsigned short),sizeof(float)})
      {
        const mh::HorizontalLaunch g=mh::horizontal_launch(p,t.max_taps,channels,quantum_bytes);
        const size_t limit=150u*1024u,budget=60u*1024u;
        const bool converted=(t.max_taps <= 8) && ((size_t) (p.max_span+p.overhang)*channels*8u <= limit);
        CHECK(g.converted == converted);
        // the class of tests/resize_cases.py; a list of up to 8 taps too wide for the converted tile runs the plain 8
        CHECK(g.maxt == (converted ? class_taps(t.max_taps) : (t.max_taps <= 8 ? 8 : class_taps(t.max_taps))));
        CHECK(g.lds_span == (converted ? p.max_span+p.overhang : p.max_span));
        const size_t row=(size_t) g.lds_span*channels*(converted ? 8u : quantum_bytes);
        CHECK(g.fits == (row <= limit));
        if (!g.fits)
          continue;
        CHECK((g.tile_rows >= 1) && (g.tile_rows <= 16));
        CHECK(g.lds == row*(size_t) g.tile_rows);
        CHECK((g.lds <= budget) || (g.tile_rows == 1));
        CHECK((g.tile_rows == 16) || ((size_t) (g.tile_rows+1)*row > budget));
      }
}

static void check(const char *name,int in,int out,double support,int expect_taps)
{
  g_name=name;
  const int before=failures;
  Table t;
  build(t,in,out,support);
  check_vertical(t);
  check_horizontal(t,expect_taps >= 0 ? expect_taps : t.max_taps);
  std::printf("%s %s %d -> %d: %d taps\n",failures == before ? "ok  " : "FAIL",name,in,out,t.max_taps);
}

int main()
{
  const double mitchell=2.0,lanczos=3.0,sinc=4.0,sharp2013=2.5,sharp2021=4.5,point=0.0;
  // TAP_CASES: (filter, source columns, target columns, largest window)
  check("mitchell <=4",37,85,mitchell,4);
  check("lanczos 5-6",37,85,lanczos,6);
  check("lanczos 7",37,37,lanczos,7);
  check("magickernelsharp2013 7",37,30,sharp2013,7);
  check("sinc 8",37,85,sinc,8);
  check("magickernelsharp2021 9-16",37,85,sharp2021,9);
  check("lanczos 9-16",37,19,lanczos,12);
  check("lanczos 17-32",37,13,lanczos,18);
  check("magickernelsharp2021 17-32",37,13,sharp2021,26);
  check("lanczos >32",300,33,lanczos,55);
  // WIDE_POINT: one or two taps, a tile too wide for the converted form at four channels
  check("wide point",5200,260,point,-1);
  {
    g_name="wide point";
    Table t;
    build(t,5200,260,point);
    mh::HorizontalPassPlan p;
    mh::build_horizontal_pass_plan(p,t);
    const mh::HorizontalLaunch g=mh::horizontal_launch(p,t.max_taps,4,sizeof(float));
    CHECK((t.max_taps <= 2) && g.fits && !g.converted && (g.maxt == 8));
  }
  // DEGENERATE_COLUMNS
  check("one column in",1,40,lanczos,-1);
  check("one column out",40,1,lanczos,-1);
  check("two columns in",2,9,lanczos,-1);
  // sizes that are no multiple of 4 or of 256, more than one tile
  check("601 outputs",300,601,lanczos,-1);
  check("1023 outputs",1100,1023,sharp2021,-1);
  // outputs without a window (count == 0): a whole tile of rows, the ends of others, a 256-column tile's first output
  {
    g_name="empty windows";
    const int before=failures;
    Table t;
    build(t,300,601,lanczos);
    for (int x : {0,5,6,7,8,9,10,11,256,257,400,600})
      t.count[x]=0;
    check_vertical(t);
    check_horizontal(t,t.max_taps);
    std::printf("%s empty windows\n",failures == before ? "ok  " : "FAIL");
  }
  std::printf(failures == 0 ? "ALL OK\n" : "%d FAILURES\n",failures);
  return failures == 0 ? 0 : 1;
}
