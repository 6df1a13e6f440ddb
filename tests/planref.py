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
