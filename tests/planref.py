"""Plain Python restatement of the stream schedule of one picture (ceracoder_amd/csrc/enc_plan.hpp) -- test infrastructure.

Transcribed from the expressions enqueue_picture() held before the schedule became a value (commit 25d698a, ceracoder_amd/csrc/enc_schedule.cpp; the
line of each is cited as [n]), not from enc_plan.hpp.  tests/test_plan_cpu.py holds plan_picture() against it on every input.
"""
MAIN, FRONT, INTRA, HANDOVER = 0, 1, 2, 3  # plan_stream_t

IN_BITS = ("idr", "all_skip", "prof", "deblock_mode", "aq_mode", "i4x4", "profile_overlap", "overlap_allowed", "exclusive_device", "wait_room0", "wait_room1",
           "keep_prefilter", "ref_flags", "pgate", "fip_rows")  # the two-valued inputs, in the order csrc/plan_driver.cpp prints them
IN_INTS = ("intra_mode", "intra_in_p", "pipeline_depth")     # ... and the three it walks over 0, 1, 2
OUT = ("may_wait", "split", "pgate", "prows", "isplit", "fip", "back", "deblock", "gpu_done", "upload_ctx", "db_follows_ip", "db_rows")


def plan(idr, all_skip, prof, deblock_mode, aq_mode, i4x4, profile_overlap, overlap_allowed, exclusive_device, wait_room0, wait_room1,
         keep_prefilter, ref_flags, pgate, fip_rows, intra_mode, intra_in_p, pipeline_depth):
    """the twelve members of pic_plan_t, in the order of OUT, as integers"""
    if all_skip:  # [182] if (all_skip) { ... } else { everything below }: no flag exists, nothing is uploaded [222 is in the else branch],
        return (0, 0, 0, 0, 0, 0, MAIN, MAIN, MAIN, 0, 0, 0)  # whatever is enqueued goes to h->stream [191-203]
    intra_p = ((2 if i4x4 and intra_in_p > 1 else 1) if intra_in_p else 0)  # [89] fill_ctx: c->intra_p
    qp_off = bool(aq_mode)                                                  # [88] fill_ctx: c->qp_off
    upload_ctx = (idr and intra_mode == 1) or deblock_mode != 0             # [222]
    may_wait = (overlap_allowed and exclusive_device and (wait_room1 if idr else wait_room0) and deblock_mode == 0 and not keep_prefilter
                and not (prof and (idr or not profile_overlap)) and not (aq_mode and intra_in_p == 2))  # [238]
    split = (not idr) and bool(intra_p) and may_wait                        # [240] (fused = true [181])
    g = (not idr) and may_wait and ref_flags and pgate                      # [248]
    prows = g and pipeline_depth >= 2                                       # [253]
    isplit = idr and intra_mode != 1 and may_wait                           # [254]
    fip = (not idr) and prows and not qp_off and bool(intra_p) and not prof and fip_rows  # [271], in the else branch of [262] if (idr)
    back = INTRA if g else MAIN                                             # [122] run_p_back: gate ? h->istream : h->stream, gate non-null with pgate [272]; [249]
    if isplit:
        deblock = INTRA                                                     # [288]
        follows, rows = False, False                                        # [288] ip_progress nullptr, after_gated_pmb defaulted to false
    elif fip:
        deblock = MAIN                                                      # [274] mst = h->stream [258]
        follows, rows = True, True                                          # [274] h->d_ip_progress, after_gated_pmb true
    else:
        deblock = MAIN                                                      # [293]
        follows, rows = split or (g and bool(intra_p)), prows               # [293]
    gpu_done = INTRA if (split or g) else MAIN                              # [281]
    return tuple(int(v) for v in (may_wait, split, g, prows, isplit, fip, back, deblock, gpu_done, upload_ctx, follows, rows))


# ---- the launches that follow from a plan (enc_plan.hpp: plan_launches).  Transcribed from what the launchers decoded out of their pointer arguments before
# launches were described by value (commit 8f135c3: enc_schedule.cpp [s n], k_deblock.hip [d n], k_motion.hip [m n]), not from enc_plan.hpp.
DB_ALL_INTRA, DB_P, DB_P_FOLLOWS_IP, DB_P_FUSED_IP = range(4)  # db_variant_t
PMB_IN_ORDER, PMB_GATED, PMB_GATED_ROWS = range(3)             # pmb_gate_t
DB_CUT_MIN_MBW, DB_ROWS = 60, 4                                # [d 986], [d 989]
LAUNCH_IN = OUT + ("idr", "qp_off", "part_words", "mbw", "mbh")
LAUNCH_OUT = ("variant", "parts", "qpc", "gate", "grid", "inc_rows", "inc_started", "inc_ip_done", "inc_qpc")
SIZES_MBW, SIZES_MBH = (1, 59, 60, 120, 512), (1, 4, 5, 9, 68, 512)


def launches(p, idr, qp_off, part_words, mbw, mbh):
    """p: the plan as a dict over OUT.  The nine members of LAUNCH_OUT."""
    # run_deblock() [s 55-57]: which arguments were non-null
    d_ip_progress, d_row_done = bool(p["db_follows_ip"]), bool(p["db_rows"])
    d_ip_strips = d_ip_done = bool(p["fip"])
    d_part_cnt = bool(part_words)                            # h->d_db_part: null under MI355ENC_NO_SPLIT [enc_handle.cpp 217]
    band0, band1 = 0, (mbh + DB_ROWS - 1) // DB_ROWS         # [s 55], [d 991]
    # k_launch_deblock_bands() [d 1027-1042]
    a_part_cnt, a_nip = False, 0                             # [d 1028], [d 1030]
    a_qpc = bool(qp_off) and band0 == 0                      # [d 1031]
    if idr:                                                  # [d 1033] h_ctx->all_intra
        variant = DB_ALL_INTRA
    else:
        a_part_cnt = band0 == 0 and mbw >= DB_CUT_MIN_MBW and d_part_cnt  # [d 1035] (band1 == nb_total: the whole picture)
        if d_ip_progress and d_ip_done and d_row_done and band0 == 0:     # [d 1037]
            variant, a_nip = DB_P_FUSED_IP, mbh                           # [d 1038-1039]
        elif d_ip_progress:
            variant = DB_P_FOLLOWS_IP                                     # [d 1041]
        else:
            variant = DB_P                                                # [d 1042]
    # launch_bands() [d 1005-1007]
    wgs = (4 if a_part_cnt else 2) * (band1 - band0)
    grid = wgs + (a_nip if a_nip > 0 else 0) + (1 if a_qpc and a_nip <= 0 else 0)
    # run_deblock() [s 58-60]: the host's totals
    inc_qpc = mbh if qp_off else 0
    inc_ip_done = mbh if p["fip"] else 0
    inc_started = wgs
    # run_p_back() [s 129-135] and k_launch_pmb()'s ladder [m 1242-1266]: `gate_done && d_row_done`, else `gate_done`, else neither
    gate_done, row_done = bool(p["pgate"]), bool(p["prows"])
    gate = PMB_GATED_ROWS if gate_done and row_done else PMB_GATED if gate_done else PMB_IN_ORDER
    inc_rows = mbw if gate_done and p["prows"] else 0        # [s 134-135]
    return (variant, int(a_part_cnt), int(a_qpc), gate, grid, inc_rows, inc_started, inc_ip_done, inc_qpc)


def wait_wgs(mbw, mbh, idr, fip_rows):
    """k_deblock_launch_wgs(mbw, mbh, idr, !idr && fip_rows) [d 995-997], as open() called it [enc_handle.cpp 162]"""
    return (4 if not idr and mbw >= DB_CUT_MIN_MBW else 2) * ((mbh + DB_ROWS - 1) // DB_ROWS) + (mbh if (not idr and fip_rows) else 0)
