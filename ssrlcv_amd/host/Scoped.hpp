// ssrlcv_amd/host/Scoped.hpp -- scope guards for the memory state of a Unity<T> argument, and the device workspace of a call.
//
// A factory method moves each Unity<T> argument to the side its C-ABI call needs, and leaves it as it came.  The three guards
// do that: construct one per argument in front of the call, and every return path is a plain return.
//
//   GpuRead<T>   the call only reads the Unity on the device (a `const T*` parameter of the C ABI)
//   GpuWrite<T>  the call writes the Unity in place on the device (a non-const device parameter)
//   CpuRead<T>   plain C++ reads the Unity's host array
//
// Contract of all three:
//   - After the scope the Unity's state equals its entry state.
//   - The side or sides that were current at entry hold the entry bytes -- for GpuWrite, the bytes the call wrote.  A read
//     guard never frees, reallocates or rewrites the side that was current: a host-resident input keeps its host array.
//   - Pinnedness is unchanged.
//   - `fore` equals the entry `fore`, with one exception: an entry of `both` with `fore` on the other side ends with
//     `fore == both` (both sides are current then).  GpuWrite on a `both` entry always ends so.
//   - Two guards on the same Unity in one scope, destroyed in reverse order, leave it as one guard would: the inner one
//     sees `both` with the needed side current and does nothing.  An argument passed twice needs no special case.
//   - A null ptr::value is allowed (an optional argument); the guard then does nothing.  A Unity in state null throws
//     NullUnityException from the constructor, as the transfer it asks for does.
//   - Guards are not copyable.
//
// entry() is the state the Unity came in: methods leave their results "in the state the points were in".
//
// DeviceScratch is the workspace of a call: max(bytes, 1) device bytes, so a zero count still has a pointer to pass, and
// bytes() as requested, so the count is passed on as 0.  The block cache (Memory.hpp) hands a freed block straight to the next
// allocation, so the destructor waits for the device before the block goes back.  Declare it after the guards of the same
// scope: it is destroyed first, and the guards then free sides no kernel still reads.
#pragma once
#include "Unity.hpp"

namespace ssrlcv {

namespace detail {
// the entry half of a guard: `side` (cpu or gpu) is made current when it is not; returns the entry state
template <typename T>
MemoryState makeCurrent(const ptr::value<Unity<T>>& u, MemoryState side) {
  if (u == nullptr) return null;
  const MemoryState entry = u->getMemoryState();
  if (u->getFore() != side && u->getFore() != both) u->transferMemoryTo(side);
  return entry;
}
}  // namespace detail

template <typename T>
class GpuRead {
  ptr::value<Unity<T>> u;
  MemoryState entered;

 public:
  explicit GpuRead(const ptr::value<Unity<T>>& unity) : u(unity), entered(detail::makeCurrent(unity, gpu)) {}
  GpuRead(const GpuRead&) = delete;
  GpuRead& operator=(const GpuRead&) = delete;
  ~GpuRead() {
    if (entered == cpu) u->clear(gpu);
  }
  MemoryState entry() const { return entered; }
};

template <typename T>
class GpuWrite {
  ptr::value<Unity<T>> u;
  MemoryState entered;

 public:
  explicit GpuWrite(const ptr::value<Unity<T>>& unity) : u(unity), entered(detail::makeCurrent(unity, gpu)) {}
  GpuWrite(const GpuWrite&) = delete;
  GpuWrite& operator=(const GpuWrite&) = delete;
  ~GpuWrite() {
    if (entered != cpu && entered != both) return;
    if (u->getFore() != gpu) u->setFore(gpu);  // the device holds the new bytes
    if (entered == cpu) u->setMemoryState(cpu);
    else u->transferMemoryTo(cpu);
  }
  MemoryState entry() const { return entered; }
};

template <typename T>
class CpuRead {
  ptr::value<Unity<T>> u;
  MemoryState entered;

 public:
  explicit CpuRead(const ptr::value<Unity<T>>& unity) : u(unity), entered(detail::makeCurrent(unity, cpu)) {}
  CpuRead(const CpuRead&) = delete;
  CpuRead& operator=(const CpuRead&) = delete;
  ~CpuRead() {
    if (entered == gpu) u->clear(cpu);
  }
  MemoryState entry() const { return entered; }
};

class DeviceScratch {
  size_t requested;
  ptr::device<unsigned char> block;

 public:
  explicit DeviceScratch(size_t bytes) : requested(bytes), block((long)(bytes ? bytes : 1)) {}
  DeviceScratch(const DeviceScratch&) = delete;
  DeviceScratch& operator=(const DeviceScratch&) = delete;
  ~DeviceScratch() { HipSafeCall(ssrlcv_hip_device_synchronize()); }
  unsigned char* get() const { return block.get(); }
  size_t bytes() const { return requested; }
};

}  // namespace ssrlcv
