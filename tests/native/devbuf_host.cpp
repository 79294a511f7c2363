// The owning device buffers of the C ABI glue (cholesky_amd/csrc/chol_devbuf.h) on the host, under the sanitizers: `make asan` builds and runs this.
// The four functions the owners are made of are defined here over malloc (exact sizes: an access past a buffer is the sanitizer's to report), with a
// switch that makes the k-th acquisition, or the next copy / clearing, fail.  A double release is AddressSanitizer's to report, a buffer never
// released LeakSanitizer's and the live count's.  No GPU, no HIP runtime.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "chol_devbuf.h"

static long g_live = 0, g_acquired = 0, g_released = 0;
static int g_fail_acquire = 0; // k > 0: the k-th acquisition from now fails (once)
static bool g_fail_fill = false; // the next copy or clearing fails (once)
int chol_dev_acquire(void **p, size_t bytes, int)
{
  *p = nullptr;
  if (g_fail_acquire > 0 && --g_fail_acquire == 0) return -5;
  if (!(*p = std::malloc(bytes ? bytes : 1))) return -5;
  g_live++; g_acquired++;
  return 0;
}
void chol_dev_release(void *p) { std::free(p); g_live--; g_released++; }
int chol_dev_zero(void *p, size_t bytes)
{
  if (g_fail_fill) { g_fail_fill = false; return -5; }
  std::memset(p, 0, bytes);
  return 0;
}
int chol_dev_copy_in(void *p, const void *host, size_t bytes)
{
  if (g_fail_fill) { g_fail_fill = false; return -5; }
  std::memcpy(p, host, bytes);
  return 0;
}

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

struct lists { dev_buf<int> a; dev_buf<double> b; int n = 0; }; // as level_dev and its siblings: buffers beside plain members
static int fill(lists &s, int n)
{
  std::vector<int> h((size_t)n, n);
  s.n = n;
  int rc = s.a.upload(h.data(), h.size());
  return rc ? rc : s.b.alloc((size_t)n);
}

// a group set up the way ensure_refine is: every buffer on its own, so that a call after a failure completes what is missing
struct group { dev_buf<long> ptr; dev_buf<double> vec, part; };
static const long g_ptr_host[4] = { 0, 3, 5, 9 };
static int ensure_group(group &g)
{
  int rc = 0;
  if (!g.ptr) rc = g.ptr.upload(g_ptr_host, 4);
  if (!rc) rc = g.vec.ensure(7);
  if (!rc) rc = g.part.ensure_zero(2);
  return rc;
}
static bool complete(const group &g) { return g.ptr && g.vec && g.part; }

static int test_moves()
{
  const long rel0 = g_released;
  dev_buf<double> a;
  CHECK(!a && a.get() == nullptr);
  CHECK(a.alloc(5) == 0 && a && g_live == 1);
  double *const pa = a;
  pa[4] = 1.0;
  dev_buf<double> b(std::move(a)); // move construction: the source is empty, nothing released
  CHECK(!a && b.get() == pa && g_live == 1 && g_released == rel0);
  dev_buf<double> c;
  CHECK(c.alloc(3) == 0 && g_live == 2);
  c = std::move(b); // move assignment: what c held is released, exactly once
  CHECK(!b && c.get() == pa && g_live == 1 && g_released == rel0 + 1);
  dev_buf<double> &cr = c;
  c = std::move(cr); // onto itself: kept
  CHECK(c.get() == pa && g_live == 1);
  CHECK(c.alloc(2) == 0 && g_live == 1 && g_released == rel0 + 2); // alloc on a held buffer releases the old one
  c.reset(); c.reset();
  CHECK(!c && g_live == 0 && g_released == rel0 + 3);
  return 0;
}
static int test_upload_ensure()
{
  dev_buf<int> u;
  const int h[3] = { 4, 5, 6 };
  CHECK(u.upload(h, 3) == 0 && u && u[0] == 4 && u[2] == 6);
  CHECK(u.upload(h, 0) == 0 && !u && g_live == 0); // no elements: empty, and what it held is released
  CHECK(u.upload(nullptr, 0) == 0 && !u);
  g_fail_fill = true;
  CHECK(u.upload(h, 3) != 0 && !u && g_live == 0); // a copy that fails leaves no half-made buffer
  g_fail_fill = true;
  CHECK(u.alloc_zero(3) != 0 && !u && g_live == 0);
  g_fail_acquire = 1;
  CHECK(u.alloc(3) != 0 && !u && g_live == 0);
  CHECK(u.alloc_zero(3) == 0 && u[0] == 0 && u[1] == 0 && u[2] == 0);
  const long acq = g_acquired;
  int *const p = u;
  CHECK(u.ensure(3) == 0 && u.ensure_zero(9) == 0 && u.get() == p && g_acquired == acq); // ensure: idempotent
  dev_buf<char> bytes; // a byte count behind a typed pointer
  CHECK(bytes.alloc_bytes(24, 1) == 0 && bytes.upload_bytes(h, sizeof h) == 0 && std::memcmp(bytes.get(), h, sizeof h) == 0 && g_live == 2);
  return 0;
}
static int test_vector()
{
  {
    std::vector<lists> v(2);
    for (int i = 0; i < 40; i++) { v.emplace_back(); CHECK(fill(v.back(), i + 1) == 0); } // grows: reallocations move the elements
    CHECK(g_live == 80 && v[41].a[0] == 40 && v[41].n == 40);
    v[5] = lists(); // reassigned: the element's buffers are released
    CHECK(g_live == 78 && !v[5].a && !v[5].b && v[5].n == 0);
    v.resize(10); // shrinks
    CHECK(g_live == 2 * 7); // elements 2..9 without element 5
    v.erase(v.begin() + 3);
    CHECK(g_live == 2 * 6 && v[3].n == 3 && v[3].a[2] == 3);
    std::vector<lists> w = std::move(v);
    CHECK(v.empty() && g_live == 2 * 6);
    w.clear();
    CHECK(g_live == 0);
    CHECK(fill(w.emplace_back(), 3) == 0);
  } // the rest goes with the container
  CHECK(g_live == 0);
  return 0;
}
static int test_group()
{
  for (int k = 1; k <= 4; k++) { // the k-th acquisition fails (k = 4: none does)
    group g;
    g_fail_acquire = k;
    int rc = ensure_group(g);
    CHECK((rc != 0) == (k <= 3));
    CHECK(rc != 0 || complete(g)); // never a success with an empty member
    CHECK(g_live == (k <= 3 ? k - 1 : 3)); // what was set up before the failure stays
    g_fail_acquire = 0;
    const long acq = g_acquired;
    CHECK(ensure_group(g) == 0 && complete(g) && g_live == 3); // the next call completes it ...
    CHECK(g_acquired == acq + (k <= 3 ? 4 - k : 0));              // ... with what was missing only
    CHECK(g.ptr[3] == 9 && g.part[0] == 0.0 && g.part[1] == 0.0);
    CHECK(ensure_group(g) == 0 && g_acquired == acq + (k <= 3 ? 4 - k : 0));
  }
  group g;
  g_fail_fill = true; // the upload's copy
  CHECK(ensure_group(g) != 0 && !g.ptr && g_live == 0);
  CHECK(ensure_group(g) == 0 && complete(g) && g.ptr[1] == 3);
  g.part.reset();
  g_fail_fill = true; // the clearing
  CHECK(ensure_group(g) != 0 && !g.part && g_live == 2);
  CHECK(ensure_group(g) == 0 && complete(g) && g_live == 3);
  return 0;
}

int main()
{
  if (test_moves() || test_upload_ensure() || test_vector() || test_group()) return 1;
  if (g_live != 0 || g_acquired != g_released) { std::fprintf(stderr, "%ld buffers live at exit (%ld acquired, %ld released)\n", g_live, g_acquired, g_released); return 1; }
  std::printf("devbuf_host: ok (%ld buffers acquired and released)\n", g_acquired);
  return 0;
}
