"""A clause 7.3.2.1.1 / E.1.1 parser of the sequence parameter sets this encoder writes: every field up to the trailing bits, the VUI's
video_signal_type included (tests/test_published_kat.py has one that insists on a VUI without it)."""


class Bits:
    def __init__(self, rbsp):
        self.b, self.pos = rbsp, 0

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.b[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + self.u(z)

    def se(self):
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)


def nal_units(stream):
    """Annex B byte stream -> [(nal_unit_type, nal_ref_idc, rbsp bytes)] (emulation prevention removed)"""
    out, i, starts = [], 0, []
    while True:
        i = stream.find(b"\x00\x00\x01", i)
        if i < 0:
            break
        starts.append(i + 3)
        i += 3
    for k, s in enumerate(starts):
        e = starts[k + 1] - 3 if k + 1 < len(starts) else len(stream)
        while e > s and stream[e - 1] == 0 and k + 1 < len(starts):
            e -= 1  # the zero_byte of the next start code
        nal = stream[s:e]
        rbsp, zeros = bytearray(), 0
        for v in nal[1:]:
            if zeros >= 2 and v == 3:
                zeros = 0
                continue
            rbsp.append(v)
            zeros = zeros + 1 if v == 0 else 0
        out.append((nal[0] & 31, nal[0] >> 5, bytes(rbsp)))
    return out


def parse_sps(rbsp):
    b, s = Bits(rbsp), {}
    s["profile_idc"], s["constraints"], s["level_idc"] = b.u(8), b.u(8), b.u(8)
    s["sps_id"] = b.ue()
    if s["profile_idc"] == 100:
        s["chroma_format_idc"], s["bit_depth_luma"], s["bit_depth_chroma"] = b.ue(), b.ue() + 8, b.ue() + 8
        assert b.u(1) == 0 and b.u(1) == 0  # qpprime_y_zero_transform_bypass_flag, seq_scaling_matrix_present_flag
    s["log2_max_frame_num"] = b.ue() + 4
    s["poc_type"] = b.ue()
    assert s["poc_type"] == 2
    s["max_num_ref_frames"], s["gaps"] = b.ue(), b.u(1)
    s["mbw"], s["mbh"] = b.ue() + 1, b.ue() + 1
    s["frame_mbs_only"], s["direct_8x8"] = b.u(1), b.u(1)
    assert s["frame_mbs_only"] == 1
    s["crop"] = (b.ue(), b.ue(), b.ue(), b.ue()) if b.u(1) else None
    assert b.u(1) == 1  # vui_parameters_present_flag
    s["sar"] = None
    if b.u(1):  # aspect_ratio_info_present_flag
        idc = b.u(8)
        s["sar"] = (b.u(16), b.u(16)) if idc == 255 else idc
    assert b.u(1) == 0  # overscan_info_present_flag
    s["video_signal_type_present"] = b.u(1)
    s["colorimetry"], s["colour_description_present"] = (0, 2, 2, 2), 0
    if s["video_signal_type_present"]:
        s["video_format"], full = b.u(3), b.u(1)
        s["colour_description_present"] = b.u(1)
        desc = (b.u(8), b.u(8), b.u(8)) if s["colour_description_present"] else (2, 2, 2)
        s["colorimetry"] = (full,) + desc
    assert b.u(1) == 0  # chroma_loc_info_present_flag
    assert b.u(1) == 1  # timing_info_present_flag
    s["num_units_in_tick"], s["time_scale"], s["fixed_frame_rate"] = b.u(32), b.u(32), b.u(1)
    assert b.u(1) == 0 and b.u(1) == 0 and b.u(1) == 0  # nal_hrd, vcl_hrd, pic_struct_present_flag
    assert b.u(1) == 1  # bitstream_restriction_flag
    s["restriction"] = (b.u(1), b.ue(), b.ue(), b.ue(), b.ue(), b.ue(), b.ue())
    assert b.u(1) == 1  # rbsp_stop_one_bit
    while b.pos & 7:
        assert b.u(1) == 0
    assert b.pos == 8 * len(rbsp), "bytes behind the trailing bits"
    return s


def sps_of(stream):
    units = nal_units(stream)
    return [parse_sps(r) for t, _, r in units if t == 7]


def slice_frame_num(slice_nal):
    """frame_num of a slice header (7.3.3: first_mb_in_slice, slice_type, pic_parameter_set_id as ue(v), then frame_num in the SPS's 8 bits); slice_nal: the
    NAL unit's bytes behind its header byte, emulation prevention still in place"""
    bits = "".join("{:08b}".format(b) for b in slice_nal.replace(b"\x00\x00\x03", b"\x00\x00")[:16])
    p = 0
    for _ in range(3):
        z = bits.index("1", p) - p
        p += 2 * z + 1
    return int(bits[p:p + 8], 2)


def slice_headers(au):
    """Per slice NAL unit of an access unit: (nal_unit_type, first_mb_in_slice, frame_num, idr_pic_id or None) -- frame_num in the 8 bits this encoder's
    SPS gives it, idr_pic_id (ue(v), IDR slices only) directly behind it (frame_mbs_only_flag = 1)"""
    out = []
    for t, _, rbsp in nal_units(au):
        if t in (1, 5):
            b = Bits(rbsp)
            first_mb, _, _ = b.ue(), b.ue(), b.ue()
            fn = b.u(8)
            out.append((t, first_mb, fn, b.ue() if t == 5 else None))
    return out
