// A small most-recently-used cache of shared values: the contribution tables of resize_filter.cpp
// and the device-side tables and plans of the resize launchers.  Host only.
//
// The cache never lets go of a value while it holds its lock: insert() and clear() hand what leaves
// to the caller, who drops it afterwards.  (A resize plan's destructor waits for the device; under
// the lock that wait would stall every other thread's lookup.)  Building a missing value is the
// caller's business too, between find() and insert(): two threads that miss the same key both
// build, and the second insert() hands the first one's value back.
//
// An object of this class is meant to be created with `new` and never destroyed: at process exit
// the runtime that the cached device blocks belong to may be gone.
#pragma once

#include <algorithm>
#include <cstddef>
#include <mutex>
#include <utility>
#include <vector>

namespace mh {

template<class Key,class Value>          // Key: operator==; Value: a std::shared_ptr
class MruCache
{
public:
  explicit MruCache(size_t capacity) : capacity_(capacity) {}
  MruCache(const MruCache &) = delete; MruCache &operator=(const MruCache &) = delete;

  // the value under `key`, now the most recent one; an empty Value when there is none
  Value find(const Key &key)
  {
    std::lock_guard<std::mutex> guard(lock_);
    return to_front(key) ? entries_.front().second : Value();
  }

  // `value` becomes the most recent entry.  Returns what left the cache for it — the value `key`
  // had, else the least recently used one of a full cache, else nothing — for the caller to drop.
  [[nodiscard]] Value insert(const Key &key,Value value)
  {
    std::lock_guard<std::mutex> guard(lock_);
    if (to_front(key))
      std::swap(entries_.front().second,value);
    else
      {
        entries_.insert(entries_.begin(),std::make_pair(key,std::move(value)));
        value=Value();
        if (entries_.size() > capacity_)
          {
            value=std::move(entries_.back().second);
            entries_.pop_back();
          }
      }
    return value;
  }

  // empties the cache; the entries are the caller's to drop
  [[nodiscard]] std::vector<std::pair<Key,Value>> clear()
  {
    std::lock_guard<std::mutex> guard(lock_);
    return std::exchange(entries_,{});
  }

  size_t size()
  {
    std::lock_guard<std::mutex> guard(lock_);
    return entries_.size();
  }

private:
  bool to_front(const Key &key)                   // (under the lock)
  {
    for (auto it=entries_.begin(); it != entries_.end(); ++it)
      if (it->first == key)
        {
          std::rotate(entries_.begin(),it,it+1);
          return true;
        }
    return false;
  }
  std::mutex lock_;
  std::vector<std::pair<Key,Value>> entries_;     // front = most recent
  const size_t capacity_;
};

} // namespace mh
