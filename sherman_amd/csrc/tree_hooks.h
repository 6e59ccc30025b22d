// tree_hooks.h — the library-internal entry points (shm__*, not part of
// include/sherman_amd.h) that one unit of the library calls in another,
// declared once: the defining unit and the caller both include this, so a
// changed signature fails to compile.  Each is documented at its definition.
#pragma once
#include <stdint.h>

#include "../../include/sherman_amd.h"

extern "C" {
// tree.cpp
uint32_t* shm__error_word(shm_tree* t);
// tree_insert.cpp
int shm__insert_batch_padded(shm_tree* t, const uint64_t* keys, const uint64_t* vals, uint64_t n,
                             void* stream);
// tree_route.cpp
int shm__route_bucket_insert(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t num_shards,
                             const uint64_t* splitters_host, uint64_t* counts_out,
                             uint64_t* keys_out, uint32_t* perm_out, void* stream);
// tree_image.cpp
int shm__export_all(shm_tree* t, uint64_t** pairs_out, uint64_t* n_out, void* stream);
// tree_read.cpp
int shm__scan_u64(shm_tree* t, const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* tot_dev,
                  void* stream);
}
