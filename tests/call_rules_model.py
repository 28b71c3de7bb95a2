"""What a whole-picture call decides on the host, restated in Python from the library's source as it stood BEFORE the rules moved
into thevc_amd/csrc/hmx_call_rules.h (issue_packed, pack_group_size and resolve_call of hmx_chain.hip, rdoq_constants of
hmx_scalar.hip).  tests/test_call_rules.py holds the header against it on the CPU, tests/test_gpu_call_rules.py the library's calls
on the GPU.  Nothing here reads the header: a rule that changes there has to be changed here by hand, with its measurement."""

RDOQ_MAX_GROUP = 2  # pictures per packing group with RDOQ: their bit-estimate tables wait in LDS
QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564)  # g_quantScales
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)  # g_invQuantScales
MAX_SIDE = 8  # side streams of a context


def pack_group(knob_group, rdoq, n_pics):
    """pack_group_size: pictures per group of the packed schedule."""
    if knob_group > 0:
        return min(knob_group, n_pics)
    if rdoq:
        return RDOQ_MAX_GROUP if n_pics >= 512 else 1
    return 4 if n_pics >= 1536 else 2 if n_pics >= 512 else 1


def pack_slots(s, slots4, slots8):
    return (slots4, slots8, 4, 1)[s]


def pack_shape(n_pics, I, knob4, knob8, rdoq, qmap, max_levels, sz, items):
    """issue_packed's geometry -> dict(n_groups, n_shards, slots4, slots8, n_rows, waves_bound, too_large)."""
    n_groups = (n_pics + I - 1) // I
    slots4 = knob4 if knob4 else (16 if 160 <= n_pics < 320 else 64)
    if qmap or rdoq:
        slots4 = 64
    if rdoq or qmap or slots4 != 64:
        slots8 = 8
    else:
        slots8 = knob8 if knob8 else (16 if n_pics >= 640 else 8)
    n_rows = max_levels * n_groups
    waves_bound = 4 * n_rows + 4 + sum(sz[s] // pack_slots(s, slots4, slots8) for s in range(4))
    too_large = items >= 0xffffffff or waves_bound >= 0x0fffffff or n_rows >= 0x7fffffff // 4
    return dict(n_groups=n_groups, n_shards=min(8, n_groups), slots4=slots4, slots8=slots8, n_rows=n_rows, waves_bound=waves_bound,
                too_large=too_large)


def pack_wave_count(knob_waves, resident, waves_bound, max_levels):
    """Persistent waves of the packed launch."""
    want = max(256, 2 * (waves_bound // max(1, max_levels)))
    return min(knob_waves, resident) if knob_waves else min(resident, want)


def resolve_schedule(resident, plan_stride, n_pics, onto, schedule=-1, across=-1, streams=0, pipeline_conv=False, graph=False):
    """resolve_call's schedule part -> (schedule, across, groups, pipelined conversions)."""
    base = 3 if resident else schedule if schedule >= 0 else 3
    packed, use_level = base == 3, base == 1
    acr = use_level and plan_stride == 0 and across != 0
    sched = 3 if packed else 0 if not use_level else (2 if acr else 1)
    groups = 1 if not acr else 3 if n_pics >= 640 else 2 if n_pics >= 384 else 1
    if use_level and streams > 0:
        groups = min(max(streams, 1), min(n_pics, MAX_SIDE))
    return sched, acr, groups, bool(pipeline_conv and acr and not graph and not onto)


def err_scale(B, q, log2n):
    """setErrScaleCoeff for flat quantiser coefficients, in the reference's operation order (IEEE double, source order)."""
    tshift = 15 - B - log2n
    return 32768.0 * 2.0 ** (-2 * tshift) / q / q / float(1 << 2 * (B - 8))


def rd_factor(iq, per, lam, B):
    """The Int64 factor of sign hiding's cost (TComTrQuant.cpp:2205)."""
    return int(iq * iq * float(1 << 2 * per) / lam / 16 / float(1 << 2 * (B - 8)) + 0.5)
