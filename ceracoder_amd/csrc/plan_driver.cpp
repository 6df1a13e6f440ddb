// plan_driver.cpp -- stand-alone driver of plan_picture() (enc_plan.hpp) for tests/test_plan_cpu.py: walks the full product of the inputs and prints one line
// of digits per input -- the fifteen two-valued inputs in the order they are set below, intra_mode, intra_in_p, pipeline_depth; a blank; the six flags, the
// three streams (plan_stream_t), upload_ctx, db_follows_ip, db_rows.  Every line is 32 bytes long.  Host code only.
#include <cstdio>

#include "enc_plan.hpp"

int main() {
    for (unsigned bits = 0; bits < (1u << 15); bits++)
        for (int t = 0; t < 27; t++) {
            const auto bit = [bits](int i) { return (bits >> i & 1u) != 0; };
            plan_in_t in;
            in.idr = bit(0); in.all_skip = bit(1); in.prof = bit(2); in.deblock_mode = bit(3); in.aq_mode = bit(4); in.i4x4 = bit(5); in.profile_overlap = bit(6);
            in.overlap_allowed = bit(7); in.exclusive_device = bit(8); in.wait_room[0] = bit(9); in.wait_room[1] = bit(10);
            in.keep_prefilter = bit(11); in.ref_flags = bit(12); in.pgate = bit(13); in.fip_rows = bit(14);
            in.intra_mode = t % 3; in.intra_in_p = t / 3 % 3; in.pipeline_depth = t / 9;
            const pic_plan_t p = plan_picture(in);
            char line[33];
            for (int i = 0; i < 15; i++) line[i] = bit(i) ? '1' : '0';
            snprintf(line + 15, sizeof line - 15, "%d%d%d %d%d%d%d%d%d%d%d%d%d%d%d\n", in.intra_mode, in.intra_in_p, in.pipeline_depth, p.may_wait, p.split, p.pgate, p.prows, p.isplit, p.fip,
                     (int)p.back, (int)p.deblock, (int)p.gpu_done, p.upload_ctx, p.db_follows_ip, p.db_rows);
            fputs(line, stdout);
        }
    return 0;
}
