// The host plan of the flat Erode / Dilate kernels (imagemagick_amd/csrc/morph_flat_plan.hpp) against what its
// tables must mean, on cell lists built here: the rectangles of widen/reach cover exactly the cells, the convex
// levels list every kernel row once under its own half-width, and rects_takes() answers as the kernel's stated
// conditions do.  Plain C++, no GPU.
#include "morph_flat_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <string>
#include <utility>

using namespace mh;

static int failures=0;
#define CHECK(cond,...) \
  do { if (!(cond)) { failures++; std::printf("FAIL %s:%d %s: ",__FILE__,__LINE__,#cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

typedef std::vector<Cell> Cells;

// every (dx,dy) of [-rx,rx] x [-ry,ry] that `inside` accepts, in raster order
static Cells from_predicate(int rx,int ry,const std::function<bool(int,int)> &inside)
{
  Cells cells;
  for (int v=-ry; v <= ry; v++)
    for (int u=-rx; u <= rx; u++)
      if (inside(u,v))
        cells.push_back(Cell{u,v,1.0});
  return cells;
}

// rows of `counts[k]` active cells centred in a kernel `width` wide, the origin at (ox,oy)
static Cells from_rows(int width,const std::vector<int> &counts,int ox,int oy)
{
  Cells cells;
  for (size_t v=0; v < counts.size(); v++)
    for (int u=(width-counts[v])/2; u < (width-counts[v])/2+counts[v]; u++)
      cells.push_back(Cell{u-ox,(int) v-oy,1.0});
  return cells;
}

static std::set<std::pair<int,int>> cell_set(const Cells &cells)
{
  std::set<std::pair<int,int>> s;
  for (const Cell &c : cells)
    s.insert(std::make_pair(c.dx,c.dy));
  return s;
}

// The conditions of morph_rects_kernel, from the cell set alone: every row between the first and the last is
// one run about the same even-summed centre, the rows mirror about the middle one and do not widen away from
// it; 16 columns of a wave's 64 (16-byte pixels) or 128 survive its 2*hmax; the (48+2*vmax)-row tile of such
// waves fits 160 KB; at most 64 distinct widths.
static bool expect_rects(const Cells &cells,size_t pixel_bytes)
{
  const std::set<std::pair<int,int>> s=cell_set(cells);
  int dy_min=1 << 30,dy_max=-(1 << 30);
  for (const auto &p : s)
    {
      dy_min=p.second < dy_min ? p.second : dy_min;
      dy_max=p.second > dy_max ? p.second : dy_max;
    }
  const int span=dy_max-dy_min+1;
  if ((span % 2) == 0)
    return false;
  std::vector<int> width((size_t) span,0),sum((size_t) span,0);
  for (const auto &p : s)
    {
      width[(size_t) (p.second-dy_min)]++;
      sum[(size_t) (p.second-dy_min)]+=p.first;
    }
  const int vmax=span/2;
  std::set<int> distinct;
  for (int k=0; k < span; k++)
    {
      const int n=width[(size_t) k];
      if ((n == 0) || ((n % 2) == 0) || (sum[(size_t) k] != n*(sum[0]/width[0])) || (sum[0] % width[0] != 0))
        return false;
      for (int u=-(n/2); u <= n/2; u++)
        if (s.count(std::make_pair(sum[(size_t) k]/n+u,k+dy_min)) == 0)
          return false;
      if (n != width[(size_t) (span-1-k)])
        return false;
      if ((k < vmax) && (n > width[(size_t) (k+1)]))
        return false;
      distinct.insert(n);
    }
  const int hmax=width[(size_t) vmax]/2;
  const int wave_columns=pixel_bytes >= 16 ? 64 : 128;
  if (wave_columns-2*hmax < 16)
    return false;
  if ((size_t) (48+2*vmax)*(size_t) wave_columns*pixel_bytes > 160u*1024u)
    return false;
  return distinct.size() <= 64;
}

// is_runs: the plan must accept the cells as centred runs.  Returns the shape for further checks.
static FlatShape check_shape(const std::string &name,const Cells &cells,bool is_runs)
{
  FlatShape s;
  const bool ok=flat_shape(cells.data(),cells.size(),s);
  CHECK(ok == is_runs,"%s: flat_shape says %d",name.c_str(),(int) ok);
  if (!ok)
    return s;
  const std::set<std::pair<int,int>> set=cell_set(cells);
  // the runs are the cells
  size_t total=0;
  for (int k=0; k < s.span; k++)
    {
      const int h=s.half[(size_t) k];
      if (h < 0)
        {
          CHECK(h == -1,"%s: empty row %d has half-width %d",name.c_str(),k,h);
          continue;
        }
      total+=(size_t) (2*h+1);
      for (int u=s.cx-h; u <= s.cx+h; u++)
        CHECK(set.count(std::make_pair(u,k+s.dy_min)) == 1,"%s: (%d,%d) is no cell",name.c_str(),u,k+s.dy_min);
    }
  CHECK(total == set.size(),"%s: %zu cells in runs, %zu in the list",name.c_str(),total,set.size());
  CHECK((s.top == (s.dy_min < 0 ? -s.dy_min : 0)) && (s.bottom == (s.dy_max > 0 ? s.dy_max : 0)),"%s: top / bottom",name.c_str());
  // widths: ascending, distinct, exactly the half-widths that occur
  std::set<int> occurring;
  for (int k=0; k < s.span; k++)
    if (s.half[(size_t) k] >= 0)
      occurring.insert(s.half[(size_t) k]);
  CHECK(std::vector<int>(occurring.begin(),occurring.end()) == s.widths,"%s: widths",name.c_str());
  CHECK(!s.widths.empty() && (s.widths.back() == s.hmax),"%s: hmax",name.c_str());
  // convex levels: every non-empty kernel row exactly once, under its own half-width
  struct { std::vector<int> level_h,level_first,level_dy; } t;
  t.level_h=s.widths;
  convex_levels(s,t.level_first,t.level_dy);
  CHECK(t.level_first.size() == t.level_h.size()+1,"%s: level_first size",name.c_str());
  CHECK((t.level_first.front() == 0) && (t.level_first.back() == (int) t.level_dy.size()),"%s: level_first ends",name.c_str());
  std::vector<int> seen((size_t) s.span,0);
  for (size_t l=0; l < t.level_h.size(); l++)
    {
      CHECK(t.level_first[l] < t.level_first[l+1],"%s: level %zu is empty",name.c_str(),l);
      for (int i=t.level_first[l]; i < t.level_first[l+1]; i++)
        {
          const int k=t.level_dy[(size_t) i]-s.dy_min;
          CHECK((k >= 0) && (k < s.span),"%s: level_dy out of the kernel",name.c_str());
          if ((k < 0) || (k >= s.span))
            continue;
          seen[(size_t) k]++;
          CHECK(s.half[(size_t) k] == t.level_h[l],"%s: row %d under half-width %d",name.c_str(),k,t.level_h[l]);
        }
    }
  for (int k=0; k < s.span; k++)
    CHECK(seen[(size_t) k] == (s.half[(size_t) k] >= 0 ? 1 : 0),"%s: row %d listed %d times",name.c_str(),k,seen[(size_t) k]);
  // rects_takes against the stated conditions
  for (size_t bytes : {(size_t) 4,(size_t) 8,(size_t) 16})
    CHECK(rects_takes(s,bytes) == expect_rects(cells,bytes),"%s: rects_takes(%zu) says %d",name.c_str(),bytes,
      (int) rects_takes(s,bytes));
  return s;
}

// the union of the rectangles of widen/reach is exactly the cell set
static void check_rectangles(const std::string &name,const Cells &cells,const FlatShape &s)
{
  struct { int nlevels; unsigned char widen[64],reach[64]; } t;
  t.nlevels=rects_levels(s,t.widen,t.reach);
  const int cy=s.dy_min+s.span/2;
  CHECK((t.nlevels >= 1) && (t.nlevels <= 64),"%s: %d levels",name.c_str(),t.nlevels);
  std::set<std::pair<int,int>> covered;
  int h=0,previous_reach=1 << 30;
  for (int l=0; l < t.nlevels; l++)
    {
      CHECK((l == 0) || (t.widen[l] > 0),"%s: level %d does not widen",name.c_str(),l);
      CHECK((int) t.reach[l] < previous_reach,"%s: reach does not fall at level %d",name.c_str(),l);
      previous_reach=t.reach[l];
      h+=t.widen[l];
      for (int v=-(int) t.reach[l]; v <= (int) t.reach[l]; v++)
        for (int u=-h; u <= h; u++)
          covered.insert(std::make_pair(s.cx+u,cy+v));
    }
  CHECK(h == s.hmax,"%s: the widenings add up to %d, hmax %d",name.c_str(),h,s.hmax);
  CHECK((int) t.reach[0] == s.span/2,"%s: the narrowest rectangle is not the tallest",name.c_str());
  CHECK(covered == cell_set(cells),"%s: %zu cells covered, %zu in the list",name.c_str(),covered.size(),cells.size());
}

static void symmetric(const std::string &name,const Cells &cells)
{
  const FlatShape s=check_shape(name,cells,true);
  // every pixel size that is taken needs the tables; the tables do not depend on it
  CHECK(s.full && ((s.span & 1) == 1),"%s: not a symmetric shape",name.c_str());
  check_rectangles(name,cells,s);
}

int main()
{
  for (int r : {1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,31})
    {
      symmetric("Disk:"+std::to_string(r),from_predicate(r,r,[r](int u,int v) { return u*u+v*v <= r*r; }));
      symmetric("Square:"+std::to_string(r),from_predicate(r,r,[](int,int) { return true; }));
      symmetric("Diamond:"+std::to_string(r),from_predicate(r,r,[r](int u,int v) { return std::abs(u)+std::abs(v) <= r; }));
      symmetric("Octagon:"+std::to_string(r),from_predicate(r,r,[r](int u,int v) { return std::abs(u)+std::abs(v) <= r+r/2; }));
      symmetric("Plus:"+std::to_string(r),from_predicate(r,r,[](int u,int v) { return (u == 0) || (v == 0); }));
    }
  {
    const Cells disk15=from_predicate(15,15,[](int u,int v) { return u*u+v*v <= 225; });
    FlatShape s;
    CHECK(disk15.size() == 709,"Disk:15 has %zu cells",disk15.size());
    CHECK(flat_shape(disk15.data(),disk15.size(),s) && (s.widths.size() == 10),"Disk:15 has %zu levels",s.widths.size());
    CHECK(rects_takes(s,4) && rects_takes(s,8) && rects_takes(s,16),"Disk:15 is taken at every pixel size");
    CHECK(rects_lds_bytes(s,8) == 79872u,"Disk:15 stages %zu bytes",rects_lds_bytes(s,8));
    const Cells disk31=from_predicate(31,31,[](int u,int v) { return u*u+v*v <= 961; });
    CHECK(flat_shape(disk31.data(),disk31.size(),s),"Disk:31");
    CHECK(rects_takes(s,4) && rects_takes(s,8) && !rects_takes(s,16),"Disk:31: 2 of a wave's 64 columns would be left");
    // wave_columns-2*hmax >= 16 on the boundary: Square:24 leaves 16 of 64, Square:25 leaves 14
    const Cells square24=from_predicate(24,24,[](int,int) { return true; }),square25=from_predicate(25,25,[](int,int) { return true; });
    CHECK(flat_shape(square24.data(),square24.size(),s) && rects_takes(s,16),"Square:24 at 16 bytes");
    CHECK(flat_shape(square25.data(),square25.size(),s) && !rects_takes(s,16) && rects_takes(s,8),"Square:25 at 16 bytes");
    // the 160 KB bound: 3 x 113 stages (48+112)*128*8 = 163840 bytes, 3 x 115 two rows more
    const Cells tall113=from_predicate(1,56,[](int,int) { return true; }),tall115=from_predicate(1,57,[](int,int) { return true; });
    CHECK(flat_shape(tall113.data(),tall113.size(),s) && rects_takes(s,8) && rects_takes(s,16),"3x113");
    CHECK(flat_shape(tall115.data(),tall115.size(),s) && rects_takes(s,4) && !rects_takes(s,8) && !rects_takes(s,16),"3x115");
  }
  // Rectangle 7x5 with its origin off the centre: symmetric about its own middle, cx and cy not 0
  {
    const Cells cells=from_rows(7,{7,7,7,7,7},1,1);
    symmetric("Rectangle:7x5+1+1",cells);
    FlatShape s;
    flat_shape(cells.data(),cells.size(),s);
    CHECK((s.cx == 2) && (s.dy_min == -1) && (s.dy_max == 3) && (s.hmax == 3),"Rectangle:7x5+1+1 geometry");
  }
  // an even number of rows: centred runs, but no middle row
  {
    const FlatShape s=check_shape("Rectangle:7x4+2+1",from_rows(7,{7,7,7,7},2,1),true);
    CHECK(s.full && !rects_takes(s,8),"Rectangle:7x4+2+1 has no middle row");
  }
  // an even width has no centre column
  check_shape("Rectangle:6x3",from_rows(6,{6,6,6},2,1),false);
  // centred runs narrowing to one side only: convex, never the rectangles
  {
    const FlatShape triangle=check_shape("triangle 5x3",from_rows(5,{1,3,5},2,1),true);
    CHECK(triangle.full && (triangle.widths == std::vector<int>{0,1,2}),"triangle 5x3 widths");
    CHECK(!rects_takes(triangle,4) && !rects_takes(triangle,8) && !rects_takes(triangle,16),"triangle 5x3 is not symmetric");
    const FlatShape trapezoid=check_shape("trapezoid 7x4",from_rows(7,{3,5,7,7},3,2),true);
    CHECK(trapezoid.full && (trapezoid.widths == std::vector<int>{1,2,3}),"trapezoid 7x4 widths");
    CHECK(!rects_takes(trapezoid,4) && !rects_takes(trapezoid,8) && !rects_takes(trapezoid,16),"trapezoid 7x4 is not symmetric");
    // symmetric, but widening away from the middle row
    const FlatShape hourglass=check_shape("hourglass 5x3",from_rows(5,{5,1,5},2,1),true);
    CHECK(!rects_takes(hourglass,8),"hourglass widens away from the middle");
  }
  // an empty row between two runs: convex lists the two rows, the rectangles need every row
  {
    Cells cells=from_rows(5,{5,0,5},2,1);
    const FlatShape s=check_shape("two bars",cells,true);
    CHECK(!s.full && (s.widths == std::vector<int>{2}) && !rects_takes(s,8),"two bars");
  }
  // a row with a gap; a run off the common centre; no cells at all
  {
    Cells gap=from_rows(5,{5,5,5},2,1);
    gap.erase(gap.begin()+7);                          // (0,0) of the middle row
    check_shape("gap",gap,false);
    Cells shifted=from_rows(5,{3,5,3},2,1);
    for (Cell &c : shifted)
      if (c.dy == 1)
        c.dx+=1;
    check_shape("shifted run",shifted,false);
    FlatShape s;
    CHECK(!flat_shape(nullptr,0,s),"no cells");
  }
  if (failures == 0)
    std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
