// The host-buffer pipeline (hostpipe.cpp): caller arrays <-> HBM in chunks through pinned staging slabs, copies
// overlapped with the kernels, and the fan-out of one call over a handle's devices.  An entry point declares its
// columns once (hostplan.h HostCols); the fan-out threshold, the shards' offsets and the slab layout all follow from
// that declaration.
#pragma once
#include <functional>

#include "hostplan.h"
#include "internal.h"

namespace msh {

// the kernels of one chunk: rows [r0, r0 + n) of the call, their columns in the device slab d
using ChunkRun = std::function<int(size_t r0, size_t n, const Slabs& d)>;

// One pipelined host call on handle t (the caller is on its device): rows [0, S) in chunks (hostplan.h host_plan, or
// plan_rows for callers whose rows are whole meshes or cameras); input columns are staged through pinned buffers and
// uploaded on a copy stream, run() enqueues the kernels on the handle's stream, and output columns come back on a
// second copy stream while the next chunk computes.  Calls of at most 16 MB make one pageable round trip instead.
int pipelined(msh_tree* t, size_t S, const HostCols& cols, const ChunkRun& run,
              const std::vector<size_t>* plan_rows = nullptr);

// Rows [0, S) of a host-buffer call over the handle and its replicas: replica g - 1 answers shard g (shard 0 stays
// here), each from its own host thread, so every device's host link and copy engines carry their share.  The shards
// are disjoint row ranges of the caller's arrays, so the answer is the one-device answer bit for bit.  call(h, r0, n)
// runs rows [r0, r0 + n) on handle h.  Calls under kFanMinBytes (32 MB) of rows stay on the handle's own device.
int fan_out(msh_tree* t, size_t S, size_t row_bytes, const std::function<int(msh_tree* h, size_t r0, size_t n)>& call);

// fan_out, then on each handle pipelined over its shard of the columns.  settle_cut: each handle first settles its
// entry cut from the whole call's S rows (each replica's automatic cut counts them all, so a G-device handle builds
// its cuts at the call a one-device handle would).
using HandleRun = std::function<int(msh_tree* h, size_t n, const Slabs& d)>;
int host_call(msh_tree* t, size_t S, const HostCols& cols, bool settle_cut, const HandleRun& run);

// the idle staging sets (the page-locked result pool is behind msh_host_alloc / msh_host_free, defined there too)
void stage_pool_trim();
void stage_pool_trim_device(int dev);  // the idle sets' device slabs of one device (the caller is on that device)
size_t stage_pool_device_bytes();

}  // namespace msh
