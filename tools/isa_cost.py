"""Static cost model of one kernel's ISA (dev tool): per basic block, instructions by issue class and an estimate of SIMD
cycles from the measured per-class issue rates (profiles/r02_measurements/valu_rates.log: cycles per wave64 instruction at
2.4 GHz with 4 waves per SIMD). Usage: tools/kernel_resources.sh; python tools/isa_cost.py [mangled-name-substring]
    python tools/isa_cost.py --loops [file.s]: of the headline kernel <0,0,1,1>, the VALU instructions by opcode of one trip of the flat leaf-box loop
(the loop over groups of eight, the block for four boxes left over, the loop over the last up to three) and of the ranked leaf loop that follows it, block
by block, then the same for the pair form (its flat loop over the 48-byte table and the leaf loop that tests a pair per trip, recognised by the four vertices
its header transforms) (the compiler's "in Loop: Header=" comments say which blocks a loop has); file.s defaults to what tools/kernel_resources.sh left, any assembly of
the MODE 1 unit will do. The pieces are found by what they contain -- a loop header with several ds_read2_b64 and v_min3_f32, a block between the two loops
with several v_min3_f32, a loop header with one ds_read_b64 triple and one v_min3_f32, the next loop header with v_ffbl_b32 -- and each is printed with its
label and its box count, so a compiler that chooses other instructions shows up as "not found" or as a count that is no multiple of the test's 11.5 per box"""
import re, sys, collections
S = "/tmp/terra_isa/render_kernels-hip-amdgcn-amd-amdhsa-gfx950.s"
LOOPS = len(sys.argv) > 1 and sys.argv[1] == "--loops"
if LOOPS:
    S = sys.argv[2] if len(sys.argv) > 2 else S
    del sys.argv[1:]
name = sys.argv[1] if len(sys.argv) > 1 else "ILi0ELi0ELi1ELi1E"
FAST = {"v_add_f32", "v_sub_f32", "v_subrev_f32", "v_mul_f32", "v_mov_b32", "v_accvgpr"}
MED = {"v_and_b32": 3.3, "v_or_b32": 3.3, "v_xor_b32": 3.4, "v_add_u32": 3.5, "v_sub_u32": 3.5, "v_subrev_u32": 3.5, "v_lshrrev_b32": 2.9, "v_fma_f32": 3.9, "v_fmac_f32": 4.1, "v_not_b32": 3.3}
TRANS = {"v_rcp_f32", "v_sqrt_f32", "v_rsq_f32", "v_exp_f32", "v_log_f32", "v_sin_f32", "v_cos_f32", "v_rcp_f64", "v_rsq_f64", "v_sqrt_f64"}
def cost(op):
    base = op.replace("_e32", "").replace("_e64", "").replace("_sdwa", "").replace("_dpp", "")
    if base in FAST: return 2.55, "fast"
    if base in MED: return MED[base], "med"
    if base in TRANS: return (16.2 if base.endswith("f64") else 8.1), "trans"
    return 4.2, "slow"
txt = open(S).read().split("\n")
start = next(i for i, l in enumerate(txt) if re.match(r"^_Z19terra_render_kernel" + name, l))


def loops_report():
    # blocks in layout order: [label, the loop header its comment names (itself for a header), instructions]
    blocks = []; cur = None
    for l in txt[start + 1:]:
        if "s_endpgm" in l: break
        m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; %bb\.(\d+):", l)
        if m:
            lab = m.group(1) if m.group(1).startswith(".") else "bb." + m.group(1)
            cur = [lab, None, []]; blocks.append(cur)
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
            if h: cur[1] = ".L" + h.group(1)
            elif "Loop Header" in l: cur[1] = lab
            continue
        if cur is None: continue
        if cur[1] is None:               # the comment may stand on the lines after the label
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
            if h and l.strip().startswith(";"): cur[1] = ".L" + h.group(1)
            elif "Loop Header" in l and l.strip().startswith(";"): cur[1] = cur[0]
        t = l.strip()
        if t and not t.startswith(";") and not t.startswith("."): cur[2].append(t.split()[0])
    def loop_of(pred, after=0):
        for i, b in enumerate(blocks):
            if i >= after and b[1] == b[0] and pred(b[2]): return i
        raise SystemExit("loop not found")
    def report(title, i):
        head = blocks[i][0]; tot = collections.Counter(); print(title + " (header " + head + ")")
        for b in blocks:
            if b[1] != head: continue
            c = collections.Counter(o.replace("_e32", "").replace("_e64", "") for o in b[2] if o.startswith("v_"))
            tot.update(c)
            print(f"  {b[0]:11s} valu {sum(c.values()):3d} lds {sum(o.startswith('ds_') for o in b[2]):2d}  " + " ".join(f"{k}x{v}" for k, v in sorted(c.items())))
        print(f"  all blocks: valu {sum(tot.values())}  " + " ".join(f"{k}x{v}" for k, v in sorted(tot.items())))
    boxes = lambda ins: sum(o.startswith("v_min3_f32") for o in ins)
    is_leaf = lambda ins: any(o.startswith("v_ffbl_b32") for o in ins)
    subs = lambda ins: sum(o.startswith("v_sub_f32") or o.startswith("v_subrev_f32") for o in ins)
    def flat_and_leaf(after, form, leaf_title, is_leaf=is_leaf):
        g = loop_of(lambda ins: ins.count("ds_read2_b64") >= 2 and boxes(ins) >= 2, after)
        report(f"{form}flat leaf-box loop, one trip over a group of {boxes(blocks[g][2])}", g)
        r = loop_of(lambda ins: "ds_read_b64" in ins and boxes(ins) == 1, g + 1)
        four = [b for b in blocks[g + 1:r] if b[1] != b[0] and boxes(b[2]) >= 2]
        if len(four) > 1: raise SystemExit("the block for the boxes left over by the groups: more than one candidate")
        if not four: print("flat leaf-box loop: no block between the two loops tests boxes (a tree with groups of four has none)")
        for b in four:
            c = collections.Counter(o.replace("_e32", "").replace("_e64", "") for o in b[2] if o.startswith("v_"))
            print(f"{form}flat leaf-box loop, the {boxes(b[2])} boxes left over by the groups (block {b[0]}, not a loop)")
            print(f"  valu {sum(c.values())}  " + " ".join(f"{k}x{v}" for k, v in sorted(c.items())))
        report(f"{form}flat leaf-box loop, one trip over a box left over", r)
        f = loop_of(is_leaf, r + 1)
        report(leaf_title, f)
        return f
    # the single form: the first flat loop of the kernel and the ranked leaf loop after it (one triangle per trip: 18 v_sub_f32 in its header)
    f = flat_and_leaf(0, "", "ranked leaf loop after it, one trip (every block, as if every branch were taken)")
    # the pair form (traverse_pairs): the flat loop whose leaf loop's header transforms four vertices (25 v_sub_f32: 12 + 8 + the 5 edge functions). Its blocks:
    # the header = the shared path to the two zero tests; sign tests and selects; determinant / depth / division, once and (behind a wave-level branch) a second
    # time for T2; the record update; then the two fallback copies of the single test, each with its double-precision block
    # (nearest first: that loop takes its first entry from the flat loop's smallest key, so its v_ffbl_b32 stands in the latch, not in the header: the header is
    # recognised by the four vertices alone -- 128 / 66 / 20 per trip with the four key instructions per box)
    groups = [i for i, b in enumerate(blocks) if b[1] == b[0] and b[2].count("ds_read2_b64") >= 2 and boxes(b[2]) >= 2]
    is_pair_leaf = lambda ins: subs(ins) >= 22
    def next_leaf(g):
        try: return loop_of(lambda ins: is_leaf(ins) or is_pair_leaf(ins), g + 1)
        except SystemExit: return None
    pair = [g for g in groups if next_leaf(g) is not None and is_pair_leaf(blocks[next_leaf(g)][2])]
    if not pair: print("pair form: no flat loop whose leaf loop transforms four vertices (a tree without the pair form has none)"); return
    flat_and_leaf(pair[0], "pair form: ", "pair form: leaf loop, one trip over a PAIR (every block, as if every branch were taken; the last blocks are the two fallback copies of the single test)", is_pair_leaf)

if LOOPS:
    loops_report(); sys.exit(0)
blocks = []; cur = ["entry", []]; blocks.append(cur)
for l in txt[start + 1:]:
    if "s_endpgm" in l: break
    m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; (%bb\.\d+):", l)      # fall-through blocks carry only a comment label
    if m: cur = [m.group(1), []]; blocks.append(cur); continue
    t = l.strip()
    if not t or t.startswith(";") or t.startswith("."): continue
    cur[1].append(t)
tot = collections.Counter(); totc = 0.0
for nm, ins in blocks:
    c = collections.Counter(); cyc = 0.0; slow = collections.Counter()
    for i in ins:
        op = i.split()[0]
        if op.startswith("v_"):
            k, cl = cost(op); cyc += k; c[cl] += 1
            if cl == "slow": slow[op.replace("_e32", "").replace("_e64", "")] += 1
        elif op.startswith("ds_"): c["lds"] += 1
        elif op.startswith("s_"): c["salu"] += 1
        else: c["mem"] += 1
    tot.update(c); totc += cyc
    if sum(c.values()) >= 12:
        print(f"{nm:11s} valu cycles {cyc:7.1f}  fast {c['fast']:3d} med {c['med']:3d} slow {c['slow']:3d} trans {c['trans']:2d} | lds {c['lds']:2d} salu {c['salu']:3d}  slow: " + " ".join(f"{k}x{v}" for k, v in slow.most_common(7)))
print("total", dict(tot), "valu cycles", round(totc))
