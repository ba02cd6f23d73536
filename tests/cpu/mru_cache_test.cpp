// MruCache (imagemagick_amd/csrc/mru_cache.hpp) with a counting value: the order of the entries, what leaves a full
// cache, WHEN a value that left is destroyed (never inside insert() or clear(): the resize launchers' plans drain the
// device in their destructors, which must not happen under the cache's lock), two builders of one key, and four
// threads over three times the capacity in keys.  Test infrastructure: built and run by tests/test_mru_cache.py (no GPU).
//   g++ -O2 -std=c++17 -pthread -I imagemagick_amd/csrc tests/cpu/mru_cache_test.cpp -o /tmp/mru_cache_test
#include "mru_cache.hpp"
#include <atomic>
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>

static std::atomic<int> g_alive{0},g_destroyed{0};
// set while the test is inside insert() or clear(): a destructor that runs then ran under the lock (or at least
// before the call returned the value to its caller)
static thread_local bool t_inside_cache=false;
static std::atomic<int> g_destroyed_inside{0};

struct Counted
{
  int key,builder;
  Counted(int k,int b) : key(k),builder(b) { g_alive++; }
  Counted(const Counted &) = delete;
  ~Counted()
  {
    g_alive--;
    g_destroyed++;
    if (t_inside_cache)
      g_destroyed_inside++;
  }
};
typedef std::shared_ptr<Counted> Value;
typedef mh::MruCache<int,Value> Cache;

static int failures=0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL line %d: %s\n",__LINE__,#cond); failures++; } } while (0)

static Value insert(Cache &cache,int key,int builder=0)
{
  Value value=std::make_shared<Counted>(key,builder);
  t_inside_cache=true;
  Value evicted=cache.insert(key,std::move(value));
  t_inside_cache=false;
  return evicted;
}

static void test_order_and_eviction()
{
  constexpr int kCapacity=4;
  Cache cache(kCapacity);
  for (int k=0; k < kCapacity; k++)
    CHECK(insert(cache,k) == nullptr);
  CHECK(cache.size() == (size_t) kCapacity);
  CHECK(cache.find(99) == nullptr);
  // a hit moves to the front: key 0 was the least recent one, now key 1 is
  CHECK((cache.find(0) != nullptr) && (cache.find(0)->key == 0));
  const int destroyed_before=g_destroyed;
  {
    Value evicted=insert(cache,kCapacity);           // capacity + 1: the least recently used entry leaves
    CHECK((evicted != nullptr) && (evicted->key == 1));
    CHECK(cache.size() == (size_t) kCapacity);
    // its destructor has not run when insert() returns ...
    CHECK(g_destroyed == destroyed_before);
    CHECK(cache.find(1) == nullptr);
    CHECK(cache.find(0) != nullptr);
  }
  // ... and has run once the returned value is dropped
  CHECK(g_destroyed == destroyed_before+1);
  // the order after find(0): 0, 4, 3, 2 — the next two insertions evict 2, then 3
  { Value e=insert(cache,10); CHECK((e != nullptr) && (e->key == 2)); }
  { Value e=insert(cache,11); CHECK((e != nullptr) && (e->key == 3)); }
  CHECK((cache.find(4) != nullptr) && (cache.find(0) != nullptr));

  // two builders of one key: the second insert() hands the first one's value back, one entry stays
  {
    insert(cache,20,1).reset();                      // (evicts one of the others)
    const int destroyed=g_destroyed;
    const size_t size=cache.size();
    Value displaced=insert(cache,20,2);
    CHECK((displaced != nullptr) && (displaced->key == 20) && (displaced->builder == 1));
    CHECK(g_destroyed == destroyed);
    CHECK(cache.size() == size);
    Value found=cache.find(20);
    CHECK((found != nullptr) && (found->builder == 2));
    displaced.reset();
    CHECK(g_destroyed == destroyed+1);
  }

  // clear() destroys nothing itself
  {
    const int destroyed=g_destroyed,alive=g_alive;
    t_inside_cache=true;
    auto released=cache.clear();
    t_inside_cache=false;
    CHECK(released.size() == (size_t) kCapacity);
    CHECK((g_destroyed == destroyed) && (g_alive == alive));
    CHECK(cache.size() == 0);
    released.clear();
    CHECK(g_destroyed == destroyed+kCapacity);
  }
  CHECK(g_alive == 0);
  CHECK(g_destroyed_inside == 0);
}

static void test_threads()
{
  constexpr int kCapacity=8,kKeys=3*kCapacity,kThreads=4,kRounds=20000;
  Cache cache(kCapacity);
  std::atomic<int> wrong{0};
  std::vector<std::thread> pool;
  for (int t=0; t < kThreads; t++)
    pool.emplace_back([&,t]()
    {
      unsigned state=12345u+977u*(unsigned) t;
      for (int i=0; i < kRounds; i++)
        {
          state=state*1664525u+1013904223u;
          const int key=(int) ((state >> 16) % (unsigned) kKeys);
          Value value=cache.find(key);
          if (value == nullptr)
            {
              Value evicted=insert(cache,key,t);
              if ((evicted != nullptr) && (evicted->key != key) && (cache.size() != (size_t) kCapacity))
                wrong++;                             // (only a full cache evicts another key's value)
              value=cache.find(key);               // (another thread may have evicted it again)
            }
          if ((value != nullptr) && (value->key != key))
            wrong++;
        }
    });
  for (std::thread &t : pool)
    t.join();
  CHECK(wrong == 0);
  CHECK(cache.size() == (size_t) kCapacity);
  // every value still alive is an entry the cache finds under its key: nothing leaked, nothing shadowed
  CHECK(g_alive == kCapacity);
  int reachable=0;
  for (int key=0; key < kKeys; key++)
    {
      Value value=cache.find(key);
      if (value != nullptr)
        {
          CHECK(value->key == key);
          reachable++;
        }
    }
  CHECK(reachable == kCapacity);
  CHECK(g_destroyed_inside == 0);
  { auto released=cache.clear(); }
  CHECK(g_alive == 0);
}

int main()
{
  test_order_and_eviction();
  test_threads();
  std::printf(failures == 0 ? "ALL OK\n" : "%d FAILURES\n",failures);
  return failures == 0 ? 0 : 1;
}
