"""The step GEMMs' prologue arguments arrive in SGPRs (kernel-argument preload, gfx950): k_gemm_ks, k_gemm_pp and k_gemm_co take what stands between wave start and their
first staging request as LEADING scalar parameters, and their translation unit is built with -amdgpu-kernarg-preload-count (ezaudio_amd/build.py UNIT_FLAGS).  (k_attn was
measured in the same form and put back: DESIGN.md section 4, "Kernel-argument preload".  The walk below knows its request -- the first vector memory load -- for the next attempt.)

Read off the gfx950 code hipcc generates today with the flags of the shipped build, for every instantiation of the three kernels that the default XL and L steps launch at
one and at four prompts (tests/golden/preload_step_kernels.txt: the kernel names of rocprofv3 kernel traces of `bench.py [--size l] [--prompts 4]`, recorded on MI355X):

  * the kernel descriptor preloads exactly the dwords of the leading set (.amdhsa_user_sgpr_kernarg_preload_length);
  * on no control-flow path from the real entry (behind the backward-compatible block that loads the same dwords from s[0:1]) to the first staging request is there an
    `s_waitcnt` that names lgkmcnt;
  * no `s_load` from the kernel-argument pointer s[0:1] on those paths has a destination that an instruction in front of the request reads.

A path has reached the request also where it branches around it (`if (this wave has a share) request`): the wave is past the point at which it would have been issued.

The first staging request: the first LDS-DMA (`global_load_lds`, `buffer_load ... lds`).

The walk is made for the step's instantiations.  In six others of the translation unit (k_gemm_pp with the plain fp32 / GEGLU epilogues, launched by kernel tests only) hipcc lays
the guarded requests out of line (the branch is TAKEN to the block with the request), which the guard rule does not recognise: there the walk reports waits behind a skipped request.

tests/test_host.py reads the ISA of gemm.hip WITHOUT the unit's flags (its helper's command line is fixed); the last test here runs those checks again on the code that ships.
"""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEADING_DWORDS = {'k_gemm_ks': 13, 'k_gemm_pp': 14, 'k_gemm_co': 14}   # 2 per pointer, 1 per int (gemm_ks.h, gemm_pp.h, gemm_co.h)
_ISA = {}


def _isa(src):
    """{mangled kernel name: its gfx950 assembly} of one translation unit, as tests/test_host.py _gfx950_isa reads it, with the unit's flags of the shipped build."""
    if src not in _ISA:
        from ezaudio_amd import build
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, src + '.s')
            subprocess.check_call([build._hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17'] + build.UNIT_FLAGS.get(src, []) +
                                  ['--cuda-device-only', '-S', os.path.join(ROOT, 'ezaudio_amd', 'csrc', src), '-o', out], stderr=subprocess.DEVNULL)
            text = open(out).read()
        _ISA[src] = {f.split(':', 1)[0]: f for f in re.split(r'\n(?=_Z\w+:)', text) if f.startswith('_Z')}
    return _ISA[src]


def _step_kernels():
    """'k_gemm_pp<128, 288, 4, 2, 3, 2, 1, 64>', ...: the step's instantiations, from the recorded traces."""
    keys = set()
    for ln in open(os.path.join(ROOT, 'tests', 'golden', 'preload_step_kernels.txt')):
        ln = ln.split('#')[0].strip()
        if ln:
            keys.add(ln)
    return keys


def _mangled_key(name):
    m = re.search(r'(k_gemm_ks|k_gemm_pp|k_gemm_co|k_attn)I((?:L[ib]\d+E)+)E', name)
    if not m:
        return None
    return m.group(1), tuple(int(x) for x in re.findall(r'L[ib](\d+)E', m.group(2)))


def _regs(tok):
    """SGPR numbers named by one operand token ('s12', 's[4:7]'), else empty."""
    m = re.fullmatch(r's(\d+)', tok)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r's\[(\d+):(\d+)\]', tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


_TWO_DESTS = re.compile(r'v_(mad_[ui]64_[ui]32|add_co|sub_co|subrev_co|addc_co|subb_co|subbrev_co|div_scale)')
_NO_DEST = ('s_cmp', 's_bitcmp', 's_cbranch', 's_branch', 's_waitcnt', 's_setreg', 's_nop', 's_barrier', 's_endpgm', 's_sleep', 's_setprio', 'global_store', 'buffer_store', 'ds_write',
            'global_load_lds', 'v_cmpx', 's_sendmsg', 's_dcache', 's_icache')


def _operands(l):
    """(SGPRs written, SGPRs read) of one instruction, from its text: the first operand is the destination (the first two of the carry-writing VALU forms), except for the
    compares, branches, stores and LDS-DMA, which only read."""
    toks = [t.rstrip(',') for t in l.split()[1:]]
    op = l.split()[0]
    nd = 0 if op.startswith(_NO_DEST) else 2 if _TWO_DESTS.match(op) else 1
    wr, rd = set(), set()
    for k, t in enumerate(toks):
        (wr if k < nd else rd).update(_regs(t))
    return wr, rd


def prologue_report(f, kind):
    """(preload length, violations, DMA instructions the walk ended at) of one kernel's assembly.  Walks EVERY control-flow path from the real entry until it meets the first
    staging request, carrying along the path the SGPRs that hold a not-yet-awaited load from the kernel-argument pointer (a join takes the union; a write to a register ends
    its pending state): a violation is an `s_waitcnt` naming lgkmcnt, or a read of such a register, on the way.  A guard -- a forward conditional branch over a STRAIGHT-LINE
    span (no label, no branch) that holds a request: `if (this wave has a share) request` -- is walked on its fall-through up to the request; its skipping side has reached the
    point of the request too and ends there.  Every other branch (the tile map's early return, the wave groups' branch) is followed on both sides."""
    pre = int(re.search(r'\.amdhsa_user_sgpr_kernarg_preload_length (\d+)', f).group(1))
    lines = [l.split(';')[0].strip() for l in f.splitlines()[1:]]
    ins = [l for l in lines if l and not l.startswith(('.p2align', '.long', '.byte', '.section', '.set', '.size', '.type', '.globl', '.amdhsa', '.end_amdhsa', '.text', '.weak', '.protected',
                                                          '.rodata', '.hidden', '.ident', '.amdgcn', '.amdgpu'))]
    label = {m.group(1): i for i, l in enumerate(ins) if (m := re.match(r'(\.LBB\d+_\d+):$', l))}
    start = 0
    if pre:   # the compatibility block: s_load from s[0:1], s_waitcnt, s_branch <real entry>
        b = next(i for i, l in enumerate(ins) if l.startswith('s_branch'))
        assert all(l.startswith(('s_load', 's_waitcnt')) for l in ins[:b]), ins[:b + 1]
        start = label[ins[b].split()[-1]]
    dma = re.compile(r'(global_load_lds|buffer_load\S* .*\blds\b)')
    anyload = re.compile(r'(global_load|buffer_load)')
    is_request = (lambda l: bool(anyload.match(l))) if kind == 'k_attn' else (lambda l: bool(dma.match(l)))

    def is_guard(i, t):
        span = ins[i + 1:t]
        return t > i and any(is_request(x) for x in span) and not any(x.endswith(':') or x.startswith(('s_branch', 's_cbranch', 's_endpgm')) for x in span)

    # The walk is path-sensitive in one more respect: hipcc merges blocks of different paths and tells them apart by a flag (`s_mov_b64 s[42:43], -1` on the way in from
    # wave group 1, `0` at the exit of group 0's loop; then `s_and_b64 vcc, exec, s[42:43]; s_cbranch_vccz <epilogue>`).  Such constants ride along, and a branch on a known
    # vcc is followed on its one feasible side -- or the walk would run from the groups' branch straight into the epilogue
    def pair(tok):
        m = re.fullmatch(r's\[(\d+):(\d+)\]', tok)
        return (int(m.group(1)), int(m.group(2))) if m and int(m.group(2)) == int(m.group(1)) + 1 else None

    bad, ended_at = [], set()
    first = (start, frozenset(), frozenset({('exec', 1)}))      # (instruction, pending kernel-argument SGPRs, known flags: ((lo, hi), 0 | -1), ('vcc', 0 | 1), ('exec', 1))
    seen, work = {first}, [first]
    while work:
        i, pend, consts = work.pop()
        pend, consts = set(pend), dict(consts)
        while i < len(ins):
            l = ins[i]
            op = l.split()[0]
            if is_request(l):
                ended_at.add(i)
                break
            if l.endswith(':'):
                i += 1
                continue
            if op == 's_waitcnt' and 'lgkmcnt' in l:
                bad.append('wait in front of the first staging request: %r (instruction %d)' % (l, i))
                pend.clear()
            wr, rd = _operands(l)
            if rd & pend:
                bad.append('%r (instruction %d) reads a kernel-argument load in front of the first staging request' % (l, i))
            pend -= wr
            if l.startswith('s_load') and re.search(r', s\[0:1\],', l):
                pend |= wr
            toks = [t.rstrip(',') for t in l.split()[1:]]
            # flags
            newc = {k: v for k, v in consts.items() if isinstance(k, str) or not (set(k) & wr)}
            if toks and toks[0] == 'vcc':
                newc.pop('vcc', None)
                if op in ('s_and_b64', 's_andn2_b64') and len(toks) == 3 and toks[1] == 'exec' and pair(toks[2]) in consts:
                    on = consts[pair(toks[2])] != 0
                    newc['vcc'] = int(on if op == 's_and_b64' else not on)      # (exec is not empty on a path a wave walks)
            elif op.startswith(('v_cmp', 'v_div_fmas', 'v_addc', 'v_subb')) and not op.endswith('_e64'):
                newc.pop('vcc', None)
            if 'saveexec' in op or op.startswith('v_cmpx') or (toks and toks[0] == 'exec'):      # exec: not empty where the wave starts; unknown behind a write, but a
                newc.pop('exec', None)                                                              # restoring `s_or_b64 exec, exec, saved` cannot empty it
                if op == 's_or_b64' and toks[:2] == ['exec', 'exec'] and 'exec' in consts:
                    newc['exec'] = 1
            if op == 's_mov_b64' and len(toks) == 2 and pair(toks[0]) and toks[1] in ('0', '-1'):
                newc[pair(toks[0])] = int(toks[1])
            consts = newc
            if op == 's_endpgm':
                break
            succ = []
            if op == 's_branch':
                succ = [label[toks[-1]]]
            elif op.startswith('s_cbranch'):
                t = label[toks[-1]]
                if op in ('s_cbranch_vccz', 's_cbranch_vccnz') and 'vcc' in consts:
                    succ = [t] if (consts['vcc'] == 0) == (op == 's_cbranch_vccz') else [i + 1]
                elif op in ('s_cbranch_execz', 's_cbranch_execnz') and 'exec' in consts:      # (hipcc's `s_cbranch_execnz next; s_branch elsewhere` behind a uniform test)
                    succ = [t] if op == 's_cbranch_execnz' else [i + 1]
                else:
                    succ = [i + 1] if is_guard(i, t) else [t, i + 1]
            if succ:
                for t in succ:
                    st = (t, frozenset(pend), frozenset(consts.items()))
                    if st not in seen:
                        seen.add(st)
                        work.append(st)
                break
            i += 1
    return pre, sorted(set(bad)), sorted(ended_at)


def _check(src, kinds, floor):
    want = _step_kernels()
    seen = set()
    for name, f in _isa(src).items():
        key = _mangled_key(name)
        if key is None or key[0] not in kinds:
            continue
        tag = '%s<%s>' % (key[0], ', '.join(str(x) for x in key[1]))
        if tag not in want:
            continue
        seen.add(tag)
        pre, bad, ended_at = prologue_report(f, key[0])
        assert pre == LEADING_DWORDS[key[0]], (tag, pre)
        assert not bad, (tag, bad[:4])
        assert ended_at, (tag, 'the walk met no LDS-DMA')
    missing = {t for t in want if t.split('<')[0] in kinds} - seen
    assert not missing, missing   # a step kernel the translation unit no longer holds under that name: re-record the list
    assert len(seen) >= floor, sorted(seen)


def test_gemm_step_kernels_reach_their_first_lds_dma_on_preloaded_arguments_only():
    _check('gemm.hip', ('k_gemm_ks', 'k_gemm_pp', 'k_gemm_co'), 19)   # 7 + 10 + 2 instantiations in the recorded traces


def test_the_walk_catches_a_wait_and_a_read_in_front_of_the_request():
    """The checker itself, on hand-made prologues."""
    head = 'k:\n\t.amdhsa_user_sgpr_kernarg_preload_length 0\n'
    dma = '\tglobal_load_lds_dwordx4 v1, s[4:5]\n'
    rep = lambda body, kind='k_gemm_ks': prologue_report(head + body, kind)
    # clean: a load in flight, a branch, the request, the wait behind it
    assert rep('\ts_load_dwordx2 s[8:9], s[0:1], 0x40\n\ts_cbranch_scc1 .LBB0_2\n\ts_add_u32 s4, s2, s3\n.LBB0_2:\n' + dma + '\ts_waitcnt lgkmcnt(0)\n\ts_endpgm\n')[1] == []
    # a wait on one side of a branch only
    assert len(rep('\ts_cbranch_scc1 .LBB0_2\n\ts_waitcnt lgkmcnt(0)\n.LBB0_2:\n' + dma + '\ts_endpgm\n')[1]) == 1
    # a kernel-argument load read by the address arithmetic; the same register re-used (written) first is no read of the load
    assert len(rep('\ts_load_dwordx2 s[8:9], s[0:1], 0x40\n\ts_add_u32 s4, s8, s3\n' + dma + '\ts_endpgm\n')[1]) == 1
    assert rep('\ts_load_dwordx2 s[8:9], s[0:1], 0x40\n\ts_mov_b32 s8, s3\n\ts_add_u32 s4, s8, s3\n' + dma + '\ts_endpgm\n')[1] == []
    assert rep('\ts_add_u32 s4, s8, s3\n\ts_load_dwordx2 s[8:9], s[0:1], 0x40\n' + dma + '\ts_endpgm\n')[1] == []      # read in FRONT of the load
    # the tile map's early return: a branch to the exit over the whole kernel.  The walk goes on behind it and finds the wait in front of the request ...
    early = '\ts_cbranch_vccnz .LBB0_9\n\ts_add_u32 s4, s2, s3\n\ts_cbranch_scc1 .LBB0_3\n%s.LBB0_3:\n' + dma + '\ts_branch .LBB0_9\n.LBB0_9:\n\ts_endpgm\n'
    assert len(rep(early % '\ts_waitcnt lgkmcnt(0)\n')[1]) == 1
    pre, bad, ended = rep(early % '\ts_nop 0\n')
    assert bad == [] and len(ended) == 1      # ... and ends AT the request when there is none
    # a guard (straight-line span with the request): the skipping side has reached the request, what follows is behind it
    guard = '\ts_cbranch_scc1 .LBB0_2\n\ts_mov_b32 m0, s13\n' + dma + '.LBB0_2:\n\ts_waitcnt lgkmcnt(0)\n\ts_endpgm\n'
    assert rep(guard)[1] == []
    # the wave groups' branch: the far side is walked too
    groups = '\ts_cbranch_scc0 .LBB0_5\n' + dma + '\ts_branch .LBB0_9\n.LBB0_5:\n\ts_waitcnt lgkmcnt(0)\n' + dma + '.LBB0_9:\n\ts_endpgm\n'
    assert len(rep(groups)[1]) == 1
    # k_attn: the query rows (a vector load) are the request
    assert rep('\ts_waitcnt vmcnt(0)\n\tglobal_load_dwordx4 v[1:4], v5, s[4:5]\n\ts_waitcnt lgkmcnt(0)\n\ts_endpgm\n', 'k_attn')[1] == []


def test_the_existing_isa_checks_of_gemm_hip_hold_on_the_code_that_ships(monkeypatch):
    """tests/test_host.py compiles gemm.hip with its own fixed flags, i.e. without kernel-argument preload: its ISA checks (no scratch, counted operand loads of k_gemm_ks, the
    step counter's scalar load, the DUAL vector, the blind statistics loads, the inline-asm MFMA wait states) see code in which the leading parameters are loaded from s[0:1].
    Here the same functions read the assembly of the shipped build."""
    from tests import test_host as TH
    monkeypatch.setitem(TH._ISA_CACHE, 'gemm.hip', _isa('gemm.hip'))
    TH.test_kernels_of_the_default_step_neither_spill_nor_shuffle_through_the_lds()
    TH.test_k_split_kernel_counts_exactly_its_operand_loads_behind_the_prologue_dma()
    TH.test_step_counter_scalar_load_is_not_touched_before_its_wait()
    TH.test_dual_form_constant_vector_registers_are_not_touched_before_their_wait()
    TH.test_blind_statistics_loads_of_the_layernorm_algebra_consumers_are_not_touched_before_their_wait()
    TH.test_inline_asm_mfma_results_are_read_behind_their_wait_states()
