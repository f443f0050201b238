// What the host decoders (vge_ingest.cpp, vge_jpeg.cpp, vge_png.cpp) share: a read-only file mapping and the pool of
// host threads that takes one item -- a video, a frame -- at a time.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/vge_ingest.h"

namespace vge {

struct Mapped {
  const uint8_t* p = nullptr;
  size_t n = 0;
  bool ok = false;  // false: unreadable, or empty
  explicit Mapped(const char* path) {
    const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return;
    struct stat st;
    if (::fstat(fd, &st) == 0 && st.st_size > 0) {
      void* m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m != MAP_FAILED) {
        p = static_cast<const uint8_t*>(m);
        n = (size_t)st.st_size;
        ok = true;
      }
    }
    ::close(fd);
  }
  ~Mapped() {
    if (ok) ::munmap(const_cast<uint8_t*>(p), n);
  }
  Mapped(const Mapped&) = delete;
  Mapped& operator=(const Mapped&) = delete;
};

// fn(i) for i in [0, n) on n_threads threads (<= 0: vge_ingest_default_threads()), at most one per item.
template <class Fn>
void parallel_for(int n, int n_threads, Fn fn) {
  int T = n_threads > 0 ? n_threads : vge_ingest_default_threads();
  T = std::max(1, std::min(T, n));
  if (T == 1) {
    for (int i = 0; i < n; ++i) fn(i);
    return;
  }
  std::atomic<int> next{0};
  std::vector<std::thread> pool;
  pool.reserve((size_t)T);
  for (int t = 0; t < T; ++t)
    pool.emplace_back([&]() {
      for (int i; (i = next.fetch_add(1)) < n;) fn(i);
    });
  for (std::thread& th : pool) th.join();
}

}  // namespace vge
