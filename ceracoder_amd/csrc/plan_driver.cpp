// plan_driver.cpp -- stand-alone driver of enc_plan.hpp and of the booking part of enc_sync.hpp for tests/test_plan_cpu.py.  Host code only.
//   (no argument)  plan_picture() over the full product of its inputs: one line of digits per input -- the fifteen two-valued inputs in the order they are set
//                  below, intra_mode, intra_in_p, pipeline_depth; a blank; the six flags, the three streams (plan_stream_t), upload_ctx, db_follows_ip, db_rows.
//                  Every line is 32 bytes long.
//   launches       plan_launches() over every distinct (plan, idr, qp_off) that walk produces x part_words x the size table: one line of integers -- the
//                  plan's twelve members, idr, qp_off, part_words, mbw, mbh; then variant, parts, qpc, gate, grid and the four increments (rows, started,
//                  ip_done, qpc).  Then, per size, idr and fip_rows, a line "room mbw mbh idr fip_rows workgroups": open()'s wait_room rule.
//   book MBW MBH   n = 2^32 / MBW + 3 pictures booked into a word_totals_t, each the two launches of a picture with the intra rows inside and then those of
//                  one with the QP_Y chain: "n", the two pictures' increments, the totals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>

#include "enc_sync.hpp"

static plan_in_t walk_input(unsigned bits, int t) {
    const auto bit = [bits](int i) { return (bits >> i & 1u) != 0; };
    plan_in_t in;
    in.idr = bit(0); in.all_skip = bit(1); in.prof = bit(2); in.deblock_mode = bit(3); in.aq_mode = bit(4); in.i4x4 = bit(5); in.profile_overlap = bit(6);
    in.overlap_allowed = bit(7); in.exclusive_device = bit(8); in.wait_room[0] = bit(9); in.wait_room[1] = bit(10);
    in.keep_prefilter = bit(11); in.ref_flags = bit(12); in.pgate = bit(13); in.fip_rows = bit(14);
    in.intra_mode = t % 3; in.intra_in_p = t / 3 % 3; in.pipeline_depth = t / 9;
    return in;
}
static int plan_digits(char *line, size_t n, const pic_plan_t &p, const char *sep) {
    const int v[12] = {p.may_wait, p.split, p.pgate, p.prows, p.isplit, p.fip, (int)p.back, (int)p.deblock, (int)p.gpu_done, p.upload_ctx, p.db_follows_ip, p.db_rows};
    int k = 0;
    for (int i = 0; i < 12; i++) k += snprintf(line + k, n - (size_t)k, "%d%s", v[i], sep);
    return k;
}
static void print_counts(const launch_counts_t &c) { printf(" %u %u %u %u", c.rows, c.started, c.ip_done, c.qpc); }

static int walk_plans() {
    for (unsigned bits = 0; bits < (1u << 15); bits++)
        for (int t = 0; t < 27; t++) {
            const plan_in_t in = walk_input(bits, t);
            char line[33];
            for (int i = 0; i < 15; i++) line[i] = (bits >> i & 1u) ? '1' : '0';
            int k = 15 + snprintf(line + 15, sizeof line - 15, "%d%d%d ", in.intra_mode, in.intra_in_p, in.pipeline_depth);
            k += plan_digits(line + k, sizeof line - (size_t)k, plan_picture(in), "");
            line[k] = '\n'; line[k + 1] = 0;
            fputs(line, stdout);
        }
    return 0;
}
static const int k_mbw[] = {1, 59, 60, 120, 512}, k_mbh[] = {1, 4, 5, 9, 68, 512};
static int walk_launches() {
    typedef std::tuple<int, int, int, int, int, int, int, int, int, int, int, int, int, int> key_t; // the plan's members, idr, qp_off
    std::set<key_t> seen;
    for (unsigned bits = 0; bits < (1u << 15); bits++)
        for (int t = 0; t < 27; t++) {
            const plan_in_t in = walk_input(bits, t);
            const pic_plan_t p = plan_picture(in);
            const key_t key(p.may_wait, p.split, p.pgate, p.prows, p.isplit, p.fip, (int)p.back, (int)p.deblock, (int)p.gpu_done, p.upload_ctx, p.db_follows_ip, p.db_rows, in.idr, in.aq_mode != 0);
            if (!seen.insert(key).second) continue;
            for (int part_words = 0; part_words < 2; part_words++)
                for (int mbw : k_mbw)
                    for (int mbh : k_mbh) {
                        const launch_shape_t l = plan_launches(p, in.idr, in.aq_mode != 0, part_words != 0, mbw, mbh);
                        char line[64];
                        plan_digits(line, sizeof line, p, " ");
                        printf("%s%d %d %d %d %d %d %d %d %d %d", line, in.idr, in.aq_mode != 0, part_words, mbw, mbh, (int)l.db, l.parts, l.qpc, (int)l.gate, l.grid);
                        print_counts(l.inc);
                        putchar('\n');
                    }
        }
    for (int mbw : k_mbw)
        for (int mbh : k_mbh)
            for (int idr = 0; idr < 2; idr++)
                for (int fip_rows = 0; fip_rows < 2; fip_rows++) printf("room %d %d %d %d %d\n", mbw, mbh, idr, fip_rows, wait_room_wgs(mbw, mbh, idr != 0, fip_rows != 0));
    return 0;
}
static int walk_bookings(int mbw, int mbh) {
    if (mbw < 1 || mbh < 1) return 2;
    pic_plan_t fused, chain; // three pictures in flight: the intra rows inside the deblocking launch / adaptive quantisation, the QP_Y chain leading it
    fused.may_wait = fused.pgate = fused.prows = fused.fip = fused.db_follows_ip = fused.db_rows = true;
    chain.may_wait = chain.pgate = chain.prows = chain.db_rows = true;
    const launch_counts_t a = plan_launches(fused, false, false, true, mbw, mbh).inc, b = plan_launches(chain, false, true, true, mbw, mbh).inc;
    const unsigned long long n = (1ull << 32) / (unsigned)mbw + 3;
    word_totals_t tot;
    for (unsigned long long i = 0; i < n; i++) { // (per picture as run_pmb() and run_deblock() book: the rows with the fused stage, the rest with the deblocking launch)
        tot.book({a.rows, 0, 0, 0}); tot.book({0, a.started, a.ip_done, a.qpc});
        tot.book({b.rows, 0, 0, 0}); tot.book({0, b.started, b.ip_done, b.qpc});
    }
    printf("%llu", n);
    print_counts(a); print_counts(b);
    print_counts({tot.rows, tot.started, tot.ip_done, tot.qpc});
    putchar('\n');
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return walk_plans();
    if (argc == 2 && !strcmp(argv[1], "launches")) return walk_launches();
    if (argc == 4 && !strcmp(argv[1], "book")) return walk_bookings(atoi(argv[2]), atoi(argv[3]));
    return 2;
}
