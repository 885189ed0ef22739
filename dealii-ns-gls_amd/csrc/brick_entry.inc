// brick_entry.inc — the first lines of gls::k_brick and gls::k_brick_sweeps
// (csrc/brick.h), ahead of the per-geometry bodies: the workgroup's brick,
// the kernel arguments its prologue needs, and the brick's record.
// Expects in scope: T, a, ENTRY_PIN.  Defines: brick, ks, k_nodes, k_target, k_coef, k_L,
// rec.  (The k_ pointers are read through load_so only.)
  // The prologue's kernel arguments in one batch: read here, ahead of
  // everything else, and pinned in scalar registers (the empty asm makes the
  // copies opaque, so every load of the batch is issued before it and waited
  // for once) instead of one scalar load and wait at each first use along the
  // prologue's dependent chain.
  BrickStreams<T> ks{a.geo_cart, a.geo_gen, a.tab_v, a.n_cells};
  const uint32_t *k_nodes = a.brick_nodes, *k_target = a.brick_target;
  const BrickRec *k_recs  = a.brick_rec;
  const T        *k_coef = a.coef;
  int             k_begin = (int)a.brick_begin, k_end = (int)a.brick_end, k_L = a.L;
  // (ENTRY_PIN false, k_brick_sweeps: plain copies; pinned, its sweep loop
  // runs out of scalar registers and spills to scratch)
  if constexpr (ENTRY_PIN)
    asm volatile(""
               : "+s"(ks.geo_cart), "+s"(ks.geo_gen), "+s"(ks.tab_v), "+s"(ks.n_cells),
                 "+s"(k_nodes), "+s"(k_target), "+s"(k_recs), "+s"(k_coef),
                 "+s"(k_begin), "+s"(k_end), "+s"(k_L));
  const int brick = k_begin + (int)blockIdx.x;
  if (brick >= k_end)
    return;
  // the brick's record: a scalar load, wave-uniform
  const BrickRec rec = brick_record(k_recs, brick);
