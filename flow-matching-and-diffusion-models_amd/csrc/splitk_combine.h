// The in-launch combine of a split reduction: the one hand-off between workgroups this library has.  Used by
// conv3x3_halo9b (8- and 4-row tiles, csrc/conv_halo9.hip), conv_igemm (csrc/conv.hip) and conv_small_kernel
// (csrc/conv_small.hip); the host side of it is ops.combine_workspace (fmdiff/runtime/ops.py).
//
// Protocol.  The `parts` workgroups of a tile each store their fp32 partial tile to their slot of the tile's slab;
// the workgroup whose ticket add came last (the reducer) reads the slots back, sums them in part order (so the sum does
// not depend on which part arrives last) and runs the epilogue; the others exit.  There is no agent-scope release or
// acquire in it.  Per-XCD L2s are not coherent with each other and a CU's vector L1 is never refreshed by another
// CU's stores, so visibility rests on the sc1 (write-through / L1-bypassing) cache policy of the payload accesses, and
// that form is valid only under four conditions (the consumer rule of the gfx950 inter-workgroup visibility notes:
// sc1 loads may stand in for the agent acquire only when all four hold):
//   (1) every load of the handed-off bytes is an sc1 buffer load to registers: combine_load() is the only reader of a
//       slab (conv_small reads all 16 slots through it and lets the descriptor's range check zero the absent ones);
//   (2) every payload byte was stored sc1: combine_store() is the only writer of a slab;
//   (3) every storing wave drains its stores (s_waitcnt vmcnt(0)) before the workgroup barrier that precedes the ONE
//       ticket add, made by lane 0 for all of the workgroup's stores: combine_drain(), then combine_ticket();
//   (4) the hand-off matches, in every cell, one measured configuration: one lane of each storing workgroup adds
//       (agent scope, relaxed) to ONE unsharded counter; the reducer is chosen by the value its own add returned;
//       its other waves load only after the barrier lane 0's wave then joins (the LDS flag + second barrier);
//       hipMalloc'ed memory; 16-byte sc1 stores and loads; ONE WORKGROUP PER CU.
// The last cell of (4) is NOT met: no caller is limited to one workgroup per CU.  By their launch bounds:
// conv3x3_halo9b 256 threads with amdgpu_waves_per_eu(2, 2): two workgroups per CU; conv_igemm
// __launch_bounds__(256, 2): two or more; conv_small_kernel __launch_bounds__(NT, 512 / NT) requests a minimum of
// 512 / NT resident workgroups (1 for NT = 512, 2 for NT = 256) and sets no maximum.  Co-resident workgroups share
// their CU's L1, which can matter only to loads that may hit L1, and (1) leaves none; the uneven-load tests
// (tests/test_gpu_halo_ticket.py, tests/test_gpu_conv_small.py) pass at these residencies.  That is reasoning and a
// test at this residency, not a match of the measured configuration: the protocol is used outside that cell.
// The whole form is measured behaviour (gfx950, ROCm 7.2), not an architectural guarantee.  The architectural
// replacement changes only this file: in combine_ticket() the lane that drew the last ticket runs
// __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent") after its add, then asm volatile("s_waitcnt vmcnt(0)"), before
// the second barrier, combine_acquire() goes, and the slots may then be read with plain loads ((2) and (3) are still
// required: the acquire repairs no producer; plain payload stores would need an agent release by lane 0 before the
// add as well).
//
// Tickets.  One counter per tile, zero at allocation; the reducer stores 0 back, so every COMPLETED launch leaves
// every ticket zero and the next launch on the stream needs no fill.  A launch that does not complete (a fault, a
// killed process) leaves them dirty: the workspace must then be dropped (ops.release_combine_workspace), not reused.
// Two launches that share tickets or slabs must not overlap: the workspace is per stream.
#pragma once
#include "common.h"

// a tile's slab of `bytes` bytes as a raw buffer (accesses past `bytes` are dropped / return zeros)
FMD_DEV auto combine_slab(float* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
}
// 16 bytes at byte offset `off` of the slab; aux 16 = sc1
template <typename R>
FMD_DEV void combine_store(R slab, int off, u32x4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, slab, off, 0, 16); }
template <typename R>
FMD_DEV u32x4 combine_load(R slab, int off) { return __builtin_amdgcn_raw_buffer_load_b128(slab, off, 0, 16); }

// The pieces of combine_is_last().  combine_drain(): every storing wave waits for its stores, then the workgroup's
// barrier.  combine_ticket(): ONE lane's add to the tile's ticket, and the reset by the one that drew the last.
FMD_DEV void combine_drain() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
FMD_DEV int combine_ticket(int* tickets, long long tile, int parts) {
  auto* tk = (__attribute__((address_space(1))) unsigned*)(tickets + tile);
  const unsigned t = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int is_last = t == (unsigned)(parts - 1);
  if (is_last) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return is_last;
}

// After this workgroup's combine_store()s: whether it is the tile's reducer (uniform over the workgroup; the others
// return from the kernel).  lds_flag: an LDS word that is dead here and that the reducer does not write before its
// next barrier.  Called by every thread of the workgroup.  (conv_igemm composes the same four lines itself:
// csrc/conv.hip says why.)
FMD_DEV bool combine_is_last(int* tickets, long long tile, int parts, int* lds_flag) {
  combine_drain();
  if (threadIdx.x == 0) *lds_flag = combine_ticket(tickets, tile, parts);
  __syncthreads();
  return *lds_flag != 0;
}
// The reducer's acquire, written by the caller directly behind its `if (!combine_is_last(...)) return;` and before its
// first combine_load(): a wavefront-scope fence, which is no instruction and only keeps the compiler from moving the
// loads above the flag.  It is a call of its own because hipcc compiles the kernels exactly as it did with the
// hand-off written out only when the fence stands behind the caller's return (inside combine_is_last() it folds that
// return into the branch that follows it).  Where the agent-acquire form replaces this one, this function goes.
FMD_DEV void combine_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
