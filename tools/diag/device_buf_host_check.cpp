// Stand-alone check of the failure path of the device-memory owner (atdn_vslam_amd/csrc/device_buf.h) for sanitizer builds,
// on a machine WITHOUT a GPU: there hipMalloc returns hipErrorNoDevice and leaves the pointer alone, so every alloc() takes
// its failing branch.
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/diag/device_buf_host_check.cpp -o check && ./check
// Exit status 0 = every expectation below held and no sanitizer report; 2 = a GPU is visible (the allocation succeeded: this
// program has nothing to say there).
#include <cstdio>
#include <utility>

#include "../../atdn_vslam_amd/csrc/device_buf.h"

namespace atdn { void set_last_error(const std::string&) {} }   // (declared by common.h; the C ABI owns the real one)

using atdn::DeviceArray;
using atdn::DeviceBuf;

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: expected %s\n", __LINE__, #cond); return 1; } } while (0)

template <class F>
static bool throws(F f) {
  try { f(); } catch (const atdn::Error&) { return true; }
  return false;
}
static bool empty(const DeviceBuf& b) { return b.p == nullptr && b.n == 0; }
static bool no_bytes() { return atdn::device_bytes_live.load() == 0; }

int main() {
  static_assert(!std::is_copy_constructible<DeviceBuf>::value && !std::is_copy_assignable<DeviceBuf>::value, "move-only");
  static_assert(std::is_nothrow_move_constructible<DeviceBuf>::value && std::is_nothrow_move_assignable<DeviceBuf>::value, "move");
  {
    DeviceBuf probe;
    if (!throws([&] { probe.alloc(16); })) { fprintf(stderr, "a GPU is visible: hipMalloc succeeded\n"); return 2; }
  }
  EXPECT(no_bytes());

  DeviceBuf a;
  EXPECT(empty(a));
  a.release();                                   // release of an empty buffer
  EXPECT(empty(a) && no_bytes());
  EXPECT(throws([&] { a.alloc(1024); }));        // a failed alloc leaves the buffer empty: no size without memory
  EXPECT(empty(a) && no_bytes());
  EXPECT(throws([&] { a.reserve(1024); }));      // ... so the same size asks again and is not "large enough"
  EXPECT(empty(a) && no_bytes());
  EXPECT(throws([&] { a.reserve(1); }));
  EXPECT(!a.reserve(0) && empty(a));             // nothing asked, nothing done
  a.release();
  EXPECT(empty(a) && no_bytes());

  // moves: the source is left empty, the target owns what the source had. No device is there to hand out a block, so the
  // "block" is a host object that is never passed to the runtime: it is taken back before anything could free it.
  static float fake[4];
  auto give = [](DeviceBuf& b) { b.p = fake; b.n = 4; };
  auto take = [](DeviceBuf& b) { b.p = nullptr; b.n = 0; };
  DeviceBuf s;
  give(s);
  DeviceBuf t(std::move(s));                     // move construction
  EXPECT(empty(s) && t.p == fake && t.n == 4);
  DeviceBuf u;
  u = std::move(t);                              // move assignment into an empty buffer
  EXPECT(empty(t) && u.p == fake && u.n == 4);
  DeviceBuf& self = u;
  u = std::move(self);                           // self-assignment keeps the block
  EXPECT(u.p == fake && u.n == 4);
  take(u);
  s = std::move(t);                              // moved-from into moved-from
  EXPECT(empty(s) && empty(t));
  s.release(); t.release();                      // release of moved-from buffers
  EXPECT(empty(s) && empty(t) && no_bytes());

  {                                              // the other element types the library uses
    DeviceArray<unsigned char> bytes;
    struct Slot { unsigned int a, b; unsigned long long c, d; };
    DeviceArray<Slot> slots;
    EXPECT(throws([&] { bytes.alloc(7); }) && bytes.p == nullptr && bytes.n == 0);
    EXPECT(throws([&] { slots.reserve(3); }) && slots.p == nullptr && slots.n == 0);
  }                                              // destruction of empty, failed and moved-from buffers: here and at return
  EXPECT(no_bytes());
  printf("device_buf.h: failed alloc leaves the buffer empty, reserve asks again, moves empty the source, 0 bytes live\n");
  return 0;
}
