// options.h — THE list of a context's tuning options: one SELLA_OPTION(name, default, rule) per option, with the
// measurements behind its default.  No include guard: internal.h includes it to make the fields of sella::Options (read
// as c->opt.NAME), context.hip to make the table behind sella_ctx_set_option / sella_ctx_get_option / sella_option_name.
// An option is added by adding a line here and nowhere else.  Rules (what the setter does with the caller's value):
//   OPT_BOOL: value ? 1 : 0 | OPT_ANY: as given | OPT_FLOOR0: negative becomes 0 | OPT_CLAMP(lo, hi): clamped into [lo, hi]
//   OPT_RANGE(lo, hi): SELLA_E_INVALID outside [lo, hi] | OPT_ONEOF(a, ...): SELLA_E_INVALID unless listed (at most 5)
// Only the setter writes c->opt: what a call needs differently for its own length is run state (host_scalars(c), internal.h).
SELLA_OPTION(gemv_rw, 0, OPT_ONEOF(0, 1, 2, 4))             // rows per workgroup in the row-panel matvec (1, 2, 4; 0 = by size: 4 from 4096 rows on, else 2)
SELLA_OPTION(gemm_mfma, 1, OPT_BOOL)                        // 1: MFMA f64 16x16x4 GEMM tiles, 0: VALU register tiles
SELLA_OPTION(host_scalars, 0, OPT_BOOL)                     // 1: host-consumed scalars are written straight into pinned host memory (measured: no gain)
SELLA_OPTION(gemm_tile128, 1, OPT_BOOL)                     // 1: 128x128 double-buffered tiles for large NN/TN products
SELLA_OPTION(eigh_leaf, 16, OPT_RANGE(2, 64))               // leaf size of the divide-and-conquer tree (16: 39.7 ms per eigh at n = 3072, 32: 40.2, 64: 41.5)
SELLA_OPTION(eigh_symv_min, 5120, OPT_RANGE(0, LONG_MAX))   // trailing blocks of at least this many rows use the symmetric-aware matvec of the
                                                            // tridiagonalisation (upper triangle only, eigh.hip); 0: never
                                                            // (with rank2k_stream the trailing update then writes the upper triangle only, mirrored once when the
                                                            // trailing block drops below this size)
SELLA_OPTION(eigh_symv_tr, 64, OPT_ONEOF(64, 128))          // rows per tile of that matvec (64 or 128)
SELLA_OPTION(eigh_nb, 16, OPT_RANGE(1, 64))                 // panel width of the blocked tridiagonalisation (tools/eigh_tune.py)
SELLA_OPTION(panel_mfma, 1, OPT_BOOL)                       // 1: products with more than 8 right-hand sides stream the matrix once (MFMA panel kernel)
SELLA_OPTION(panel_rows, 0, OPT_ONEOF(0, 16, 32, 48, 64))   // rows per workgroup of the panel kernel: 16, 32, 48, 64, or 0 = by size (one workgroup per CU)
SELLA_OPTION(eigh_wy_mfma, 1, OPT_BOOL)                     // 1: back-transformation on the matrix cores, 0: VALU/LDS variant
SELLA_OPTION(dav_fuse_scale, 1, OPT_BOOL)                   // Davidson chain: (d - theta)^-1 scaling in the epilogue of the residual kernel (0: own kernel)
SELLA_OPTION(dav_poll, 1, OPT_BOOL)                         // ... 1: the fused iteration's one wait polls a sequence word in pinned host memory, written by a
                                                            //    one-thread kernel behind the iteration's last kernel (the scalars of the iteration are then
                                                            //    stored there by their kernels for the length of the call), instead of sleeping on an event — the wake-up of an interrupt-driven wait is
                                                            //    ~10 us of a ~95 us iteration
SELLA_OPTION(dav_zero_copy, 0, OPT_BOOL)                    // ... its coefficients read from pinned host memory instead of a copy launch (measured equal or slower)
SELLA_OPTION(eigh_tail_lds, 128, OPT_FLOOR0)                // trailing blocks of at most this many rows (<= 128) are tridiagonalised by one workgroup in LDS (0: never)
SELLA_OPTION(eigh_wy_nb64_min, 2560, OPT_ANY)               // 64 instead of 32 reflectors per block of the back-transformation from this many rows on (0: never)
SELLA_OPTION(eigh_wy_rows, 16, OPT_ANY)                     // rows of X per workgroup of the MFMA back-transformation (16, or 32: two row tiles)
SELLA_OPTION(eigh_wy_waves, 4, OPT_ANY)                     // wavefronts per workgroup of the MFMA back-transformation (4, 8 or 16: measured equal at n = 3072 and 12288 — the kernel is bound by L2 bandwidth, 22.7 GB in 3.16 ms, not by latency)
SELLA_OPTION(lr_cholqr, 1, OPT_BOOL)                        // 1: block of update vectors orthonormalised by Cholesky-QR twice (eigh.hip, lr_lowrank_update)
SELLA_OPTION(h2d_kernel_min, 16384, OPT_FLOOR0)             // host-to-device payloads of at least this many bytes are copied by a kernel reading the pinned ring (0: never)
SELLA_OPTION(eigh_dc_pipeline, 1, OPT_BOOL)                 // 1: divide & conquer queues the next level's rank-one vectors behind the current level (one wait per level)
SELLA_OPTION(eigh_gemv_flat, 1, OPT_BOOL)                   // 1: trailing matvec of the tridiagonalisation with every load issued before the first wait (eigh.hip)
SELLA_OPTION(eigh_wy_strip, 1, OPT_ANY)                     // 1: back-transformation with the strip of X in registers for the whole sweep (n = ld a multiple of 64,
                                                            //    2048 < n <= 3072: 2.49 -> 2.19 ms, L2 traffic 19.9 -> 14.5 GB); 2: any such n <= 3072 (tests); 0: never
SELLA_OPTION(rank2k_fixed, 1, OPT_BOOL)                     // 1: trailing update with all loads issued up front for the panel depths 16 / 32 (update.hip)
SELLA_OPTION(rs_fast, 1, OPT_BOOL)                          // 1: sella_opt_step searches the restricted step by interpolating batches (stepper.hip)
SELLA_OPTION(lr_dev, 1, OPT_BOOL)                           // 1: sella_opt_step updates structured decompositions in coordinates, all decisions on the device (lrstep.hip)
SELLA_OPTION(rank2k_stream, 1, OPT_BOOL)                    // 1: trailing update of the tridiagonalisation as a mirror-free MFMA stream (update.hip)
SELLA_OPTION(panel_small, 2048, OPT_FLOOR0)                 // panel products with <= 64 rows and at least this many columns split the long index over the
                                                            // chip (kernels.hip); 0: never
SELLA_OPTION(dav_rotate_fused, 1, OPT_BOOL)                 // sella_davidson's result stage: rotation into the Ritz basis and the caller's layout in one launch (k <= 32)
SELLA_OPTION(bd_early_matvec, 1, OPT_BOOL)                  // pipelined block Davidson: 1 = A applied to the raw correction block while the host orthonormalises it
                                                            // (A T by the same coefficients as T, error budget; see davidson_block.hip), 0 = A applied to the final T
SELLA_OPTION(bd_pipeline, 1, OPT_BOOL)                      // block Davidson: pipelined iteration (davidson_block.hip run_pipelined: A applied to the raw correction
                                                            // block while the host does the SVQB step, two polled waits per iteration); 0: the general loop
SELLA_OPTION(eigh_wy_overlap, 1, OPT_BOOL)                  // 1: Gram matrices / triangular factors of the compact-WY blocks on a second stream, beside divide & conquer
SELLA_OPTION(eigh_upd_max, 1024, OPT_CLAMP(0, 8 * 1024 - 64))  // trailing blocks of at most this many rows are tridiagonalised with ONE launch per column, the block
                                                            //    kept up to date by the launch itself (trd_upd_kernel, eigh.hip); 0: never.  eigh at n = 3072 by
                                                            //    switch-over size (session r05b): 0: 39.85 ms, 512: 38.78, 1024: 38.28, 1536: 39.07, 2048: 40.19,
                                                            //    3072: 47.9 — the block is written back once per column, which only pays while it is small
                                                            //    (clamped: one launch per column is at most 1024 workgroups of at most 8 rows, eigh.hip TRD_UPD_MAXGRID — larger
                                                            //    blocks stay with the blocked chain instead of failing in the middle of a factorisation)
SELLA_OPTION(eigh_upd_rows, 0, OPT_ONEOF(0, 2, 4, 8))       // rows per workgroup of that kernel (2, 4, 8); 0: 2 (measured best at every size up to 1024)
SELLA_OPTION(eigh_upd_nt, 512, OPT_ONEOF(128, 256, 512))    // most threads per workgroup of that kernel (128, 256, 512; tests force several chunks per thread with 128)
SELLA_OPTION(emt_hcap, 8, OPT_ANY)                          // neighbour-list slots per thread of the EMT kernels (tests: 1 forces the overflow path)
SELLA_OPTION(lr_overlap, 0, OPT_BOOL)                       // 1: the view job of the one-call step is queued on a second stream, beside the coordinate kernels of the
                                                            //    full-space job.  Measured (session r04k): EMT-slab step 0.59-0.62 ms either way, and the ensemble of EMT
                                                            //    members DROPS from 211 to 172-182 searches/s with 8 threads x 2 streams: off
SELLA_OPTION(rs_batch_result, 1, OPT_BOOL)                  // 1: on an expected boundary step the start value rides in the first batch and the final step is read from the
                                                            //    batch that produced it (stepper.hip)
SELLA_OPTION(lr_pipe, 1, OPT_BOOL)                          // 1: the library search queues the force call in front of the update that consumes it: one wait for both (search.hip)
SELLA_OPTION(lr_chain, 1, OPT_BOOL)                         // 1: the O(n r) passes of the one-call step as five fused launches, merged coordinate kernels (lrstep.hip)
SELLA_OPTION(rs_hint, 1, OPT_BOOL)                          // 1: the batched root search interpolates quadratically through three evaluated points and, given the alpha the
                                                            //    previous root search of the same saddle search ended at (sella_opt_step_t::alpha_hint), looks around it first:
                                                            //    4.9 -> 3.5 rounds per boundary step on the EMT slab
SELLA_OPTION(gs_small, 2048, OPT_CLAMP(0, 2048))            // Gram-Schmidt of vectors of at most this many entries (<= 2048) in ONE launch of one workgroup, sweeps,
                                                            //    norms and accept / drop decisions included (gs.hip); 0: always the sweep-by-sweep launches
SELLA_OPTION(rs_batch, 1, OPT_BOOL)                         // 1: bisection phase of the restricted-step root find evaluates 15 trial alphas per round trip (stepper.hip)
