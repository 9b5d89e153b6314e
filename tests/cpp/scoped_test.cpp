// tests/cpp/scoped_test.cpp -- (GPU) the scope guards and the scratch of ssrlcv_amd/host/Scoped.hpp against the contract at the top
// of that header: every entry condition of a Unity<float> of 5 values and of 1, for GpuRead, GpuWrite and CpuRead; two guards
// nested; a null argument; the scratch.  Device allocations and copies only, no kernel.  One "ok ..." line a case, "done" last.
#include <cstdio>
#include <cstring>
#include <vector>
#include "ssrlcv.hpp"

using namespace ssrlcv;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_case); return false; } \
  } while (0)

static char g_case[96] = "";

struct Entry {
  const char* name;
  MemoryState state, fore;
  bool pinned;
};
static const Entry kEntries[] = {
    {"cpu", cpu, cpu, false},           {"cpu-pinned", cpu, cpu, true},     {"gpu", gpu, gpu, false},
    {"both-fore-cpu", both, cpu, false}, {"both-fore-gpu", both, gpu, false}, {"both-fore-both", both, both, false},
};

typedef ptr::value<Unity<float>> UnityF;

static std::vector<float> series(unsigned long n, float first) {
  std::vector<float> v(n);
  for (unsigned long i = 0; i < n; ++i) v[i] = first + (float)i;
  return v;
}
static bool hostIs(const UnityF& u, const std::vector<float>& want) {
  return u->host.get() != nullptr && std::memcmp(u->host.get(), want.data(), want.size() * sizeof(float)) == 0;
}
static bool deviceIs(const UnityF& u, const std::vector<float>& want) {
  if (u->device.get() == nullptr) return false;
  std::vector<float> got(want.size());
  HipSafeCall(ssrlcv_hip_memcpy(got.data(), u->device.get(), want.size() * sizeof(float), 1));
  return std::memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0;
}
static void writeDevice(const UnityF& u, const std::vector<float>& values) {
  HipSafeCall(ssrlcv_hip_memcpy(u->device.get(), values.data(), values.size() * sizeof(float), 0));
}

// a Unity in the entry condition `e`: `current` are the bytes of the side that is current, `stale` those of the other side of a
// `both` entry whose fore is one side (equal to current everywhere else)
static UnityF make(const Entry& e, unsigned long n, std::vector<float>& current, std::vector<float>& stale) {
  const std::vector<float> first = series(n, 1.5f), newer = series(n, 100.25f);
  UnityF u(nullptr, n, cpu, e.pinned);
  std::memcpy(u->host.get(), first.data(), n * sizeof(float));
  current = stale = first;
  if (e.state == gpu) u->setMemoryState(gpu);
  if (e.state == both) u->transferMemoryTo(gpu);
  if (e.state == both && e.fore == cpu) {  // the host is made newer after the transfer
    std::memcpy(u->host.get(), newer.data(), n * sizeof(float));
    u->setFore(cpu);
    current = newer;
  }
  if (e.state == both && e.fore == gpu) {  // the device is made newer
    writeDevice(u, newer);
    u->setFore(gpu);
    current = newer;
  }
  return u;
}

static bool entryHolds(const UnityF& u, const Entry& e) {
  CHECK(u->getMemoryState() == e.state && u->getFore() == e.fore && u->isPinned() == e.pinned);
  return true;
}

// after a read guard for `side`: the state, fore, pinnedness, pointers and bytes of the contract
static bool afterRead(const UnityF& u, const Entry& e, MemoryState side, const float* hostBefore, const float* deviceBefore,
                      const std::vector<float>& current, const std::vector<float>& stale) {
  const MemoryState other = side == gpu ? cpu : gpu;
  CHECK(u->getMemoryState() == e.state && u->isPinned() == e.pinned);
  CHECK(u->getFore() == (e.state == both && e.fore == other ? both : e.fore));
  if (e.state != both) {  // one-sided: the kept side is the same array, the other side is gone
    CHECK(u->host.get() == hostBefore && u->device.get() == deviceBefore);
    CHECK(e.state == cpu ? (u->device.get() == nullptr && hostIs(u, current)) : (u->host.get() == nullptr && deviceIs(u, current)));
    return true;
  }
  // both: the side that was current was not rewritten; the other holds the same bytes unless it was never asked for
  const bool refreshed = e.fore == other, untouchedStale = e.fore == side;
  CHECK(side == gpu ? deviceIs(u, current) : hostIs(u, current));
  if (refreshed || e.fore == both) CHECK(hostIs(u, current) && deviceIs(u, current));
  if (untouchedStale) CHECK(side == gpu ? hostIs(u, stale) : deviceIs(u, stale));
  CHECK(u->host.get() == hostBefore && u->device.get() == deviceBefore);
  return true;
}

template <typename Guard>
static bool readCase(const Entry& e, unsigned long n, MemoryState side) {
  std::vector<float> current, stale;
  UnityF u = make(e, n, current, stale);
  if (!entryHolds(u, e)) return false;
  const float *hostBefore = u->host.get(), *deviceBefore = u->device.get();
  {
    Guard guard(u);
    CHECK(guard.entry() == e.state);
    CHECK(side == gpu ? deviceIs(u, current) : hostIs(u, current));
  }
  return afterRead(u, e, side, hostBefore, deviceBefore, current, stale);
}

static bool writeCase(const Entry& e, unsigned long n) {
  std::vector<float> current, stale;
  const std::vector<float> written = series(n, -7.75f);
  UnityF u = make(e, n, current, stale);
  if (!entryHolds(u, e)) return false;
  {
    GpuWrite<float> guard(u);
    CHECK(guard.entry() == e.state);
    CHECK(deviceIs(u, current));
    writeDevice(u, written);
  }
  CHECK(u->getMemoryState() == e.state && u->isPinned() == e.pinned);
  CHECK(u->getFore() == (e.state == both ? both : e.fore));
  if (e.state == cpu) CHECK(u->device.get() == nullptr && hostIs(u, written));  // the new bytes reached the host
  if (e.state == gpu) CHECK(u->host.get() == nullptr && deviceIs(u, written));
  if (e.state == both) CHECK(hostIs(u, written) && deviceIs(u, written));
  return true;
}

// two guards on one Unity, destroyed in reverse order, leave it as one guard would
template <typename Guard>
static bool nestedCase(const Entry& e, unsigned long n, MemoryState side, bool writes) {
  std::vector<float> current, stale;
  const std::vector<float> written = series(n, -7.75f);
  UnityF u = make(e, n, current, stale);
  const float *hostBefore = u->host.get(), *deviceBefore = u->device.get();
  {
    Guard outer(u);
    {
      Guard inner(u);
      CHECK(outer.entry() == e.state && inner.entry() == (e.state == side ? e.state : both));  // the inner one has nothing to do
      CHECK(side == gpu ? deviceIs(u, current) : hostIs(u, current));
      if (writes) writeDevice(u, written);
    }
    CHECK(u->getMemoryState() == (e.state == side ? e.state : both));
    CHECK(side == gpu ? deviceIs(u, writes ? written : current) : hostIs(u, current));
  }
  CHECK(u->getMemoryState() == e.state && u->getFore() == e.fore && u->isPinned() == e.pinned);
  if (writes) {
    CHECK(e.state == cpu ? (u->device.get() == nullptr && hostIs(u, written)) : (u->host.get() == nullptr && deviceIs(u, written)));
    return true;
  }
  return afterRead(u, e, side, hostBefore, deviceBefore, current, stale);
}

static bool nullCase() {
  UnityF none;
  {
    GpuRead<float> a(none);
    GpuWrite<float> b(none);
    CpuRead<float> c(none);
    CHECK(a.entry() == null && b.entry() == null && c.entry() == null);
  }
  CHECK(none == nullptr);
  bool threw = false;  // a Unity in state null is refused as the transfer it asks for refuses it
  try {
    UnityF empty;
    empty.construct();
    GpuRead<float> a(empty);
  } catch (NullUnityException&) {
    threw = true;
  }
  CHECK(threw);
  return true;
}

static bool scratchCase() {
  {
    DeviceScratch none(0);
    CHECK(none.get() != nullptr && none.bytes() == 0);
  }
  DeviceScratch some(300);
  CHECK(some.get() != nullptr && some.bytes() == 300);
  std::vector<unsigned char> pattern(300, 0xA5), back(300, 0);  // at least 300 bytes are there to write and read
  HipSafeCall(ssrlcv_hip_memcpy(some.get(), pattern.data(), 300, 0));
  HipSafeCall(ssrlcv_hip_memcpy(back.data(), some.get(), 300, 1));
  CHECK(back == pattern);
  return true;
}

int main() {
  const unsigned long sizes[2] = {5, 1};
  for (unsigned long n : sizes)
    for (const Entry& e : kEntries) {
      std::snprintf(g_case, sizeof g_case, "gpu-read %s n=%lu", e.name, n);
      if (!readCase<GpuRead<float>>(e, n, gpu)) return 1;
      std::printf("ok %s\n", g_case);
      std::snprintf(g_case, sizeof g_case, "gpu-write %s n=%lu", e.name, n);
      if (!writeCase(e, n)) return 1;
      std::printf("ok %s\n", g_case);
      std::snprintf(g_case, sizeof g_case, "cpu-read %s n=%lu", e.name, n);
      if (!readCase<CpuRead<float>>(e, n, cpu)) return 1;
      std::printf("ok %s\n", g_case);
    }
  for (const Entry& e : kEntries) {
    if (e.state == both || e.pinned) continue;  // nesting: a cpu and a gpu entry
    std::snprintf(g_case, sizeof g_case, "nested gpu-read %s", e.name);
    if (!nestedCase<GpuRead<float>>(e, 5, gpu, false)) return 1;
    std::printf("ok %s\n", g_case);
    std::snprintf(g_case, sizeof g_case, "nested gpu-write %s", e.name);
    if (!nestedCase<GpuWrite<float>>(e, 5, gpu, true)) return 1;
    std::printf("ok %s\n", g_case);
    std::snprintf(g_case, sizeof g_case, "nested cpu-read %s", e.name);
    if (!nestedCase<CpuRead<float>>(e, 5, cpu, false)) return 1;
    std::printf("ok %s\n", g_case);
  }
  std::snprintf(g_case, sizeof g_case, "null argument");
  if (!nullCase()) return 1;
  std::printf("ok %s\n", g_case);
  std::snprintf(g_case, sizeof g_case, "scratch");
  if (!scratchCase()) return 1;
  std::printf("ok %s\n", g_case);
  std::printf("done\n");
  return 0;
}
