// What the launchers of csrc/k_*.hip share on the host side: the device's CU count, one resident round of workgroups, the dynamic-LDS
// limit, and the table of a kernel family's built instantiations.
#pragma once
#include <climits>
#include <cstddef>

namespace dq {

// Compute units of the current device, queried once per process (256 where the query fails: no device).  (dq_api.hip)
int device_cus();
// One resident round of `fn` at (threads, dynamic LDS bytes): occ_blocks_per_cu(...) * device_cus().  Returns < 0 after set_error().
int resident_blocks(const void* fn, int threads, size_t lds);
// Raises fn's dynamic-LDS limit to `bytes` (launches above 48 KB), once per (function, device).  Returns 0, or 1 after set_error().
int ensure_dynamic_lds(const void* fn, size_t bytes);

// One built instantiation of a kernel template: its template arguments as integers, and the kernel.  A family's `static const` array of
// these is the only statement of what is built: the family's predicate and its launcher both read it.
template <class Fn, int NK>
struct Inst {
  int key[NK];
  Fn fn;
};
// a row from the kernel template's name and its arguments, written once: the key cannot disagree with the kernel
#define DQ_INST(KERNEL, ...) {{__VA_ARGS__}, KERNEL<__VA_ARGS__>}

// The first row whose key matches, or nullptr.  `any`: a value that, standing in a row's key, matches every call (a family whose template
// takes one argument value to mean "decided at run time" passes that value and puts those rows after the exact ones).
template <class Fn, int NK, size_t R>
const Inst<Fn, NK>* find_inst(const Inst<Fn, NK> (&table)[R], const int (&key)[NK], int any = INT_MIN) {
  for (const Inst<Fn, NK>& r : table) {
    bool hit = true;
    for (int i = 0; i < NK; ++i) hit = hit && (r.key[i] == key[i] || r.key[i] == any);
    if (hit) return &r;
  }
  return nullptr;
}

}  // namespace dq
