// Stand-alone host check of densecap_amd/csrc/scratch.h: the header's runtime calls are replaced by the counting stand-ins below
// (DC_SCRATCH_STANDIN), which log every call in order.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_scratch_host.py; exits 0 and prints "scratch_host ok" when every property holds.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
typedef int hipStream_t;

static std::vector<std::string> g_log;
static bool g_fail_malloc = false;
static hipError_t hipMalloc(void** p, size_t bytes) {
  if (g_fail_malloc) { g_log.push_back("malloc-failed"); return hipErrorOutOfMemory; }
  *p = malloc(bytes ? bytes : 1);
  g_log.push_back("malloc " + std::to_string(bytes));
  return hipSuccess;
}
static hipError_t hipFree(void* p) {
  g_log.push_back("free");
  free(p);
  return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t s) {
  g_log.push_back("sync " + std::to_string(s));
  return hipSuccess;
}
static const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e == hipSuccess ? "no error" : "invalid value"; }

#define DC_SCRATCH_STANDIN
#include "../densecap_amd/csrc/scratch.h"

static int g_bad = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
  } while (0)

static bool log_is(std::initializer_list<const char*> want) {
  std::vector<std::string> w(want.begin(), want.end());
  if (w == g_log) return true;
  printf("  log:");
  for (const auto& l : g_log) printf(" [%s]", l.c_str());
  printf("\n");
  return false;
}

// the host layer's fail path in small: a context that keeps the message, and the early-returning macro of its call sites
struct Ctx {
  ScratchStats scratch;
  std::string err;
  int fail(int code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
};
#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return ctx->fail(-3, "%s failed: %s", #expr, hipGetErrorString(_e));    \
  } while (0)

// a call in the host layer's shape: a scoped block, then work that may refuse
static int a_call(Ctx* ctx, hipStream_t s, bool refuse, int64_t* live_inside) {
  Scratch block(ctx->scratch, s);
  HIPCHK(block.alloc(1000));
  *live_inside = ctx->scratch.live;
  if (refuse) return ctx->fail(-1, "refused");
  return 0;
}

int main() {
  Ctx c;
  Ctx* ctx = &c;
  int64_t live = -1;

  // normal exit: one sync of the call's stream, then the one free
  g_log.clear();
  EXPECT(a_call(ctx, 7, false, &live) == 0);
  EXPECT(live == 1 && c.scratch.live == 0);
  EXPECT(log_is({"malloc 1000", "sync 7", "free"}));

  // early return: the same
  g_log.clear();
  EXPECT(a_call(ctx, 9, true, &live) == -1 && c.err == "refused");
  EXPECT(live == 1 && c.scratch.live == 0);
  EXPECT(log_is({"malloc 1000", "sync 9", "free"}));

  // a failed allocation: reported through the fail path, nothing to drain or free, nothing counted
  g_log.clear();
  g_fail_malloc = true;
  live = -1;
  EXPECT(a_call(ctx, 7, false, &live) == -3);
  g_fail_malloc = false;
  EXPECT(c.err == "block.alloc(1000) failed: out of memory");
  EXPECT(live == -1 && c.scratch.live == 0);
  EXPECT(log_is({"malloc-failed"}));

  // a block that never allocates touches nothing; a second allocation is refused
  g_log.clear();
  { Scratch none(c.scratch, 3); EXPECT(none.get() == nullptr); }
  EXPECT(log_is({}));
  {
    Scratch twice(c.scratch, 3);
    EXPECT(twice.alloc(16) == hipSuccess && twice.alloc(16) == hipErrorInvalidValue && c.scratch.live == 1);
  }
  EXPECT(c.scratch.live == 0);
  EXPECT(log_is({"malloc 16", "sync 3", "free"}));

  // carve: 256-byte pieces in list order; a zero-byte piece takes no room, 257 bytes take two pieces
  {
    void *p0 = nullptr, *p1 = nullptr, *p2 = nullptr, *p3 = nullptr, *p4 = nullptr;
    const std::vector<Carve> cv = {{&p0, 100}, {&p1, 0}, {&p2, 256}, {&p3, 257}, {&p4, 1}};
    EXPECT(carve(cv, nullptr) == 256 + 0 + 256 + 512 + 256);
    EXPECT(p0 == nullptr && p4 == nullptr);                    // base = null: only the bytes
    g_log.clear();
    {
      Scratch block(c.scratch, 5);
      EXPECT(block.alloc(cv) == hipSuccess);
      char* b = static_cast<char*>(block.get());
      EXPECT(p0 == b && p1 == b + 256 && p2 == b + 256 && p3 == b + 512 && p4 == b + 1024);
      static_cast<char*>(p4)[255] = 1;                         // the last byte of the block is the block's
    }
    EXPECT(log_is({"malloc 1280", "sync 5", "free"}));
  }

  // the kept buffer: grows only, drains before it replaces, counts
  {
    g_log.clear();
    KeptBuf k(c.scratch);
    EXPECT(k.get() == nullptr && k.bytes() == 0);
    EXPECT(k.grow(1000, 4) == hipSuccess);
    void* first = k.get();
    EXPECT(first != nullptr && k.bytes() == 1000 && c.scratch.kept_bytes == 1000 && c.scratch.kept_allocs == 1);
    EXPECT(log_is({"malloc 1000"}));
    EXPECT(k.grow(1000, 4) == hipSuccess && k.grow(10, 4) == hipSuccess);     // fits: kept, nothing called
    EXPECT(k.get() == first && k.bytes() == 1000 && c.scratch.kept_allocs == 1);
    EXPECT(log_is({"malloc 1000"}));
    g_log.clear();
    EXPECT(k.grow(1001, 6) == hipSuccess);                                    // does not fit: drain, free, allocate
    EXPECT(log_is({"sync 6", "free", "malloc 1001"}));
    EXPECT(k.bytes() == 1001 && c.scratch.kept_bytes == 1001 && c.scratch.kept_allocs == 2);
    g_log.clear();
    EXPECT(k.grow(500, 6) == hipSuccess && k.bytes() == 1001 && c.scratch.kept_allocs == 2);   // back to a smaller request
    EXPECT(log_is({}));
    // a replacement that fails leaves an empty buffer, not a stale pointer
    g_fail_malloc = true;
    EXPECT(k.grow(5000, 6) == hipErrorOutOfMemory);
    g_fail_malloc = false;
    EXPECT(k.get() == nullptr && k.bytes() == 0 && c.scratch.kept_bytes == 0 && c.scratch.kept_allocs == 2);
    EXPECT(log_is({"sync 6", "free", "malloc-failed"}));
    g_log.clear();
    EXPECT(k.grow(64, 6) == hipSuccess && c.scratch.kept_bytes == 64 && c.scratch.kept_allocs == 3);
    KeptBuf other(c.scratch);
    EXPECT(other.grow(36, 6) == hipSuccess && c.scratch.kept_bytes == 100);
    other.reset();
    EXPECT(other.get() == nullptr && c.scratch.kept_bytes == 64);
    other.reset();                                                            // (idempotent)
    EXPECT(log_is({"malloc 64", "malloc 36", "free"}));
    g_log.clear();
  }
  EXPECT(log_is({"free"}));                                                   // k's destructor
  EXPECT(c.scratch.kept_bytes == 0 && c.scratch.live == 0);

  if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
  printf("scratch_host ok\n");
  return 0;
}
