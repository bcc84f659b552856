"""What the generators of the hand-scheduled MFMA statements share (tools/gen_bf16_trunk.py, gen_bf16_chain.py, gen_x3_trunk.py,
gen_x3_chain.py; the weight-gradient generators gen_dw_*.py use write_asm_macro only).

One design: a BACKBONE of MFMAs in execution order; FILLERS (release gap, deadline, cost) dealt into the gap behind each MFMA by a
list scheduler, earliest deadline first, under a per-gap issue budget; counted waits and hazard padding tracked on the emitted text.
  Filler     one non-MFMA instruction (or a sync point) with its scheduling window
  Emitter    the emitted text + the state the counted waits and the s_nop padding are derived from
  Backbone   slab / k-step / MFMA numbering
  Scheduler  owns the fillers; run() walks the backbone and calls the generator's issue_mfma(i, entry) for each MFMA
A generator keeps what is its kernel's: knobs, register plan, slab geometry, filler builders, preamble and issue_mfma.
"""
import re


class Filler:
    __slots__ = ("text", "cost", "release", "deadline", "kind", "reads", "writes", "tag", "seq")
    def __init__(self, text, cost, release, deadline, kind, reads=(), writes=(), tag=None):
        self.text, self.cost, self.release, self.deadline, self.kind = text, cost, release, deadline, kind
        self.reads, self.writes, self.tag = set(reads), set(writes), tag
        self.seq = 0


class Emitter:
    def __init__(self, vm_on_entry, dma_thin=1, dma_exec=0):
        """vm_on_entry: issue-order tags of the LDS-DMA pieces that may still be in flight when the statement starts (older memory
        operations of the kernel only make the first counted waits stricter: vmcnt retires in order).  dma_thin / dma_exec: timing
        experiments (WRONG results) -- issue only every dma_thin-th piece / run every DMA with EXEC = %[em]."""
        self.out = []                 # emitted instruction texts
        self.lgkm = []                # outstanding LDS reads (tags) in issue order
        self.vm = list(vm_on_entry)   # outstanding vector-memory operations (tags) in issue order
        self.dma_thin, self.dma_exec, self.dma_seen = dma_thin, dma_exec, 0
        self.last_salu_write = {}     # SGPR -> wait-state clock of the SALU instruction that wrote it (SALU -> VMEM address: 5 states)
        self.last_valu_write = {}     # reg -> index in self.out of the VALU instruction that wrote it
        self.n_states = 0             # wait states issued so far (every instruction = 1, s_nop n = n + 1)
        self.state_at = []            # wait-state clock of each emitted instruction
        self.last_m0 = -10
        self.mfma_count = 0
        self.stats = dict(nop=0, wait=0, forced=0)

    # ---- raw emission --------------------------------------------------------------------------------------------
    def emit(self, text, writes=(), valu=False, states=1):
        self.out.append(text)
        self.state_at.append(self.n_states)
        if valu:
            for r in writes:
                self.last_valu_write[r] = self.n_states
        self.n_states += states

    def mfma(self, text):
        self.emit(text, states=8)
        self.mfma_count += 1

    def salu_mov(self, sreg, src):
        """s_mov_b32 of an operand into a physical SGPR of the statement (a running pointer), tracked for the SALU -> VMEM distance"""
        self.emit("s_mov_b32 s%d, %s" % (sreg, src))
        self.last_salu_write[sreg] = self.n_states - 1

    def ds_read(self, text, tag):
        self.emit(text)
        self.lgkm.append(tag)

    def nop(self, n):                 # n wait states
        while n > 0:
            c = min(n, 8)
            self.emit("s_nop %d" % (c - 1), states=c)
            self.stats["nop"] += 1
            n -= c

    def pad_valu_to_mfma(self, regs):
        """VALU write -> MFMA read of the same register needs 2 wait states in between."""
        need = 0
        for r in regs:
            w = self.last_valu_write.get(r)
            if w is not None:
                need = max(need, 3 - (self.n_states - w))      # writer at clock w; reader must be at >= w + 3
        if need > 0:
            self.nop(need)

    def pad_valu_to_swap(self, regs):
        """VALU write -> v_permlane32_swap_b32 read of the same register: 2 wait states (what hipcc inserts for its own code)."""
        self.pad_valu_to_mfma(regs)

    def pad_salu_to_vmem(self, sregs):
        need = 0
        for r in sregs:
            w = self.last_salu_write.get(r)
            if w is not None:
                need = max(need, 6 - (self.n_states - w))
        if need > 0:
            self.nop(need)

    def wait_lgkm(self, tags):
        """counted wait: every LDS read carrying one of `tags` has returned (LDS reads return in order)."""
        pos = -1
        for i, t in enumerate(self.lgkm):
            if t in tags:
                pos = i
        if pos < 0:
            return
        n = len(self.lgkm) - 1 - pos
        assert n <= 15, "lgkmcnt field is 4 bits"
        self.emit("s_waitcnt lgkmcnt(%d)" % n)
        self.stats["wait"] += 1
        del self.lgkm[:pos + 1]

    def wait_vm(self, tag):
        """counted wait on the vector-memory queue (retires in issue order): the operation carrying `tag` has completed.  The count
        field has 6 bits: a target with more than 63 younger operations is covered by vmcnt(63) (at most the 63 youngest remain)."""
        if tag not in self.vm:
            return
        pos = max(i for i, t in enumerate(self.vm) if t == tag)
        self.emit("s_waitcnt vmcnt(%d)" % min(63, len(self.vm) - 1 - pos))
        self.stats["wait"] += 1
        del self.vm[:pos + 1]

    def run_filler(self, f):
        k = f.kind
        if k == "ds_read":
            self.ds_read(f.text, f.tag)
        elif k == "vload":                               # global load into registers of the statement (waited for with wait_vm)
            self.pad_salu_to_vmem(f.reads)
            self.emit(f.text)
            self.vm.append(f.tag)
        elif k == "valu":
            if f.tag is not None:                        # needs LDS data (sigma weights) / a loaded register (("vm", tag))
                if f.tag[0] == "vm":
                    self.wait_vm(f.tag[1])
                else:
                    self.wait_lgkm({f.tag})
            self.emit(f.text, writes=f.writes, valu=True)
        elif k == "ds_write":
            self.emit(f.text)
            self.lgkm.append(("stw",))
        elif k == "swap":
            self.pad_valu_to_swap(f.reads)
            self.emit(f.text, writes=f.writes, valu=True)
        elif k == "salu":
            self.emit(f.text)
            for r in f.writes:
                self.last_salu_write[r] = self.n_states - 1
        elif k == "vstore":
            if f.tag is not None:                        # the staged row has arrived in its registers
                self.wait_lgkm({f.tag})
            self.pad_salu_to_vmem(f.reads)
            self.emit(f.text)
            self.vm.append(10 ** 9)                      # never the target of a counted wait: only ever counts as "younger"
        elif k == "m0":
            self.emit(f.text)
            self.last_m0 = self.n_states - 1
        elif k == "dma":
            if self.n_states - self.last_m0 < 2:         # s_mov m0 -> LDS-DMA: one wait state
                self.nop(1)
            self.dma_seen += 1
            if self.dma_seen % self.dma_thin == 0:
                if self.dma_exec:
                    self.emit("s_mov_b64 exec, %[em]")
                self.emit(f.text)
                if self.dma_exec:
                    self.emit("s_mov_b64 exec, -1")
                self.vm.append(f.tag)
        elif k == "bar":
            # own pieces of the NEXT slab have landed (later slabs may still be in flight: counted vmcnt), then all waves meet
            nxt = f.tag
            pos = -1
            for i, t in enumerate(self.vm):
                if isinstance(t, int) and t <= nxt:
                    pos = i
            if pos >= 0:
                self.emit("s_waitcnt vmcnt(%d)" % min(63, len(self.vm) - 1 - pos))   # (6-bit field: a larger count only waits for more)
                del self.vm[:pos + 1]
            self.emit("s_barrier")
        else:
            self.emit(f.text)


class Backbone:
    """The MFMAs in execution order: mf[i] = (slab, k-step, j), j < per_kstep (point tile / term of the 3-term split);
    gk[(slab, k-step)] = global k-step index, kstep_list its inverse; first[slab] = index of the slab's first MFMA (first[n_slabs] =
    len(mf)); idx_of[mf[i]] = i."""
    def __init__(self, n_slabs, nk_of, per_kstep):
        self.n_slabs = n_slabs
        self.mf, self.gk, self.first, self.kstep_list = [], {}, {}, []
        for s in range(n_slabs):
            self.first[s] = len(self.mf)
            for ks in range(nk_of(s)):
                self.gk[(s, ks)] = len(self.kstep_list)
                self.kstep_list.append((s, ks))
                self.mf.extend((s, ks, j) for j in range(per_kstep))
        self.first[n_slabs] = len(self.mf)
        self.idx_of = {m: i for i, m in enumerate(self.mf)}


class Scheduler:
    """The list scheduler.  Epilogue builders hand over ITEMS (kind, text, writes, tag, cls[, reads]): cls "acc" = reads the slab's
    accumulator set (deadline: before slab s + 2 overwrites it), "post" = works on packed words / LDS / memory only (deadline one slab
    later; same-deadline items keep their program order, so a slab's post items still run before the next slab's accumulator items)."""
    def __init__(self, emitter, dma_cost, valu_cost, lds_cost, salu_cost):
        self.g = emitter
        self.cost = {"ds_read": lds_cost, "ds_write": lds_cost, "valu": valu_cost, "swap": valu_cost, "vstore": dma_cost,
                     "salu": salu_cost, "m0": salu_cost, "dma": dma_cost}
        self.fillers, self.pending = [], []       # pending: released, not yet emitted
        self.n_added = self.n_released = 0

    def add(self, f):
        f.seq = self.n_added
        self.n_added += 1
        self.fillers.append(f)
        return f

    def as_filler(self, item, rel, dl):
        kind, text, writes, tag, _cls = item[:5]
        reads = item[5] if len(item) > 5 else ()
        return Filler(text, self.cost[kind], rel, dl, kind, reads=reads, writes=writes, tag=tag)

    @staticmethod
    def keep_program_order(fillers):
        """`fillers` is ONE program-ordered sequence (packed-word registers, sign words, the staging tile, row buffers and running
        offsets are reused from tile to tile): deadlines must not decrease along it, or the list scheduler (earliest deadline first)
        would let a later tile's work overtake an earlier tile's"""
        for a, b in zip(reversed(fillers[:-1]), reversed(fillers[1:])):
            if a.deadline > b.deadline:
                a.deadline = b.deadline
                a.release = min(a.release, a.deadline)

    def add_deferred_epilogues(self, bb, flat_of, rel_off, handover, program_order=True):
        """The epilogue of slab s (items flat_of(s)) runs inside slab s + 1, from rel_off MFMAs behind the slab's last one (results
        readable), at least two items per gap.  handover(s) = index of the first MFMA that READS what the epilogue writes into the
        other activation set, where that comes before the accumulator deadline (only the LAST tile of a layer is read soon), else
        None.  Returns the last slab's items: they are flushed behind the backbone (finish)."""
        N, first, last = bb.n_slabs, bb.first, len(bb.mf) - 1
        epi = []
        for s in range(N - 1):
            flat = flat_of(s)
            acc_dl = first[s + 2] - 1 if s + 2 < N else last
            post_dl = first[s + 3] - 1 if s + 3 < N else last
            if handover(s) is not None:
                acc_dl = min(acc_dl, handover(s) - 2)
            per_gap = max(2, -(-len(flat) // max(1, first[s + 2] - first[s + 1] - 4)))
            for j, item in enumerate(flat):
                d = acc_dl if item[4] == "acc" else max(acc_dl, post_dl)
                epi.append(self.add(self.as_filler(item, min(first[s + 1] + rel_off + j // per_gap, d), d)))
        if program_order:
            self.keep_program_order(epi)
        return flat_of(N - 1)

    def weight_stream_piece(self, m0_text, rel, dl, tag, bump=4096, rewind=None):
        """one 4 KB LDS-DMA piece of the weight stream: LDS destination into m0, the load, the address bump (dependent fillers: they
        sit next to each other in this order, see run).  rewind: the stream wraps -- back by that many bytes in front of the load."""
        self.add(Filler(m0_text, self.cost["m0"], rel, dl, "m0"))
        if rewind is not None:
            self.add(Filler("v_subrev_u32 %%[goff], %d, %%[goff]" % rewind, self.cost["valu"], rel, dl, "valu", writes=("goff",)))
        self.add(Filler("global_load_lds_dwordx4 %[goff], %[blob]", self.cost["dma"], rel, dl, "dma", tag=tag))
        self.add(Filler("v_add_u32 %%[goff], %d, %%[goff]" % bump, self.cost["valu"], rel, dl, "valu", writes=("goff",)))

    def release(self, upto):
        while self.n_released < len(self.fillers) and self.fillers[self.n_released].release <= upto:
            self.pending.append(self.fillers[self.n_released])
            self.n_released += 1
        self.pending.sort(key=lambda f: (f.deadline, f.seq))

    def pop_ready(self, cap):
        """the gap behind an MFMA: pending fillers in (deadline, seq) order while the issue budget lasts.  STRICT order: the
        first filler that does not fit closes the gap (dependent fillers -- m0 / DMA / address bump, cvt / max / write -- sit
        next to each other in this order and must never overtake one another)."""
        budget, n = cap, 0
        for f in self.pending:
            if budget < f.cost - 1e-9:
                break
            self.g.run_filler(f); budget -= f.cost; n += 1
        self.pending = self.pending[n:]

    def run(self, backbone, issue_mfma, cap):
        """backbone: the MFMAs in execution order; issue_mfma(i, entry) emits the operand waits, the hazard padding and the MFMA; cap:
        the issue budget of a gap"""
        self.fillers.sort(key=lambda f: (f.release, f.seq))
        for i, entry in enumerate(backbone):
            self.release(i - 1)
            n = 0                                        # forced fillers (deadline = before this MFMA)
            while n < len(self.pending) and self.pending[n].deadline <= i - 1:
                self.g.run_filler(self.pending[n]); self.g.stats["forced"] += 1; n += 1
            self.pending = self.pending[n:]
            issue_mfma(i, entry)
            self.release(i)
            self.pop_ready(cap)

    def finish(self, tail_states, epi_tail):
        """behind the backbone: everything still pending, the last slab's epilogue (MFMA results readable after tail_states wait
        states), every LDS read returned"""
        self.release(float("inf"))
        for f in self.pending:
            self.g.run_filler(f)
        self.pending = []
        self.g.nop(tail_states)
        for item in epi_tail:
            self.g.run_filler(self.as_filler(item, 0, 0))
        if self.g.lgkm:
            self.g.emit("s_waitcnt lgkmcnt(0)")
            self.g.lgkm = []


def interleave(a, b):
    """deal list b evenly into list a (both keep their own order)"""
    if not b:
        return list(a)
    out, j = [], 0
    for i, x in enumerate(a):
        out.append(x)
        while j < len(b) and (j + 1) * len(a) <= (i + 1) * len(b):
            out.append(b[j]); j += 1
    return out + b[j:]


def parse_knobs(argv, KNOBS):
    """knob=value ... over the defaults KNOBS; a value takes the type of its default, an unknown knob is an error"""
    knobs = dict(KNOBS)
    for kv in argv:
        k, v = kv.split("=")
        if k not in KNOBS:
            raise KeyError(k)
        knobs[k] = float(v) if isinstance(KNOBS[k], float) else int(v)
    return knobs


def write_asm_macro(f, name, lines):
    """#define name as the concatenation of one C string per instruction"""
    f.write("#define %s \\\n" % name)
    for line in lines:
        f.write('  "%s\\n\\t" \\\n' % line)
    f.write('  ""\n')


def write_inc(path, g, prefix, header, v_first=128):
    """the emitted stream as a C string macro <prefix>_ASM + the clobber list <prefix>_CLOBBERS.  VGPRs / SGPRs: exactly the physical
    registers the text names, v_first = first VGPR the statement may own (a shorter fragment ring etc. hands registers back to the
    compiler).  AGPRs: the WHOLE file, so that the compiler can never park a value in an AGPR across the statement (under register
    pressure it otherwise hoists loop invariants into a0.., which the next tile reads back after the statement has overwritten them --
    tools/check_agpr.py flags any compiler-allocated AGPR for the same reason)."""
    n_other = len(g.out) - g.mfma_count
    used, sused = set(), set()
    for line in g.out:
        for m in re.finditer(r"\bv\[(\d+):(\d+)\]", line):
            used.update(range(int(m.group(1)), int(m.group(2)) + 1))
        for m in re.finditer(r"\bv(\d+)\b", line):
            used.add(int(m.group(1)))
        for m in re.finditer(r"\bs\[(\d+):(\d+)\]", line):
            sused.update(range(int(m.group(1)), int(m.group(2)) + 1))
        for m in re.finditer(r"\bs(\d+)\b", line):
            sused.add(int(m.group(1)))
    with open(path, "w") as f:
        f.write("// GENERATED by %s -- do not edit.\n" % header)
        f.write("// %d MFMAs, %d other instructions (%.2f per MFMA): %d s_nop, %d counted waits\n"
                % (g.mfma_count, n_other, n_other / g.mfma_count, g.stats["nop"], g.stats["wait"]))
        write_asm_macro(f, prefix + "_ASM", g.out)
        assert used and min(used) >= v_first, "the statement only names registers of its own range"
        f.write("#define %s_CLOBBERS " % prefix + ", ".join('"v%d"' % r for r in sorted(used)) + ", "
                + "".join('"s%d", ' % r for r in sorted(sused))
                + ", ".join('"a%d"' % r for r in range(256)) + ', "memory", "scc"\n')


def summary_line(name, g):
    n_other = len(g.out) - g.mfma_count
    return ("%s: %d MFMAs, %d other (%.2f / MFMA), nops %d, waits %d, forced %d"
            % (name, g.mfma_count, n_other, n_other / g.mfma_count, g.stats["nop"], g.stats["wait"], g.stats["forced"]))
