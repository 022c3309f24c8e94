"""Static instruction counts of one kernel in a gfx950 assembly listing:

  hipcc <build.py FLAGS> -DDX_SPEC_ONLY=DxSpec_shadow_reorient -S --cuda-device-only \\
      dexterity_amd/csrc/dx_step.hip -o step.s
  python tools/asm_counts.py step.s dx_step_kernel_queue_spec

counts the instructions between the first label that contains the name and its s_endpgm
block's end (.Lfunc_end), by class, and prints the kernel's register report."""
import collections
import re
import sys


def kernel_lines(path: str, name: str):
    body, inside = [], False
    for line in open(path, errors="replace"):
        s = line.strip()
        if not inside:
            if re.match(rf"^[\w.$]*{re.escape(name)}[\w.$]*:", s) and not s.startswith(".L"):
                inside = True
            continue
        if s.startswith(".Lfunc_end"):
            break
        body.append(s)
    return body


def classify(op: str) -> str:
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "global"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path, name = sys.argv[1], sys.argv[2]
    ops = []
    for s in kernel_lines(path, name):
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        ops.append(s.split()[0])
    c = collections.Counter(classify(o) for o in ops)
    n = collections.Counter(ops)
    pre = lambda p: sum(v for k, v in n.items() if k.startswith(p))  # noqa: E731
    print(f"kernel {name}: {len(ops)} instructions")
    for k in ("valu", "mfma", "salu", "smem", "lds", "global", "other"):
        print(f"  {k:8s} {c[k]:7d}  ({100.0 * c[k] / max(len(ops), 1):.1f} %)")
    print(f"  s_cbranch_execz/execnz {n['s_cbranch_execz'] + n['s_cbranch_execnz']}, s_cbranch_* {pre('s_cbranch')}, "
          f"s_and_saveexec_b64 {n['s_and_saveexec_b64']}, *_saveexec_* {sum(v for k, v in n.items() if 'saveexec' in k)}")
    print(f"  s_waitcnt {n['s_waitcnt']}, s_nop {n['s_nop']}, v_writelane_b32 {n['v_writelane_b32']}, "
          f"v_readlane_b32 {n['v_readlane_b32']}, v_cndmask_b32 {pre('v_cndmask_b32')}, ds_write* {pre('ds_write')}, "
          f"ds_read* {pre('ds_read')}")
    # writers of exec: the destination (first operand) is exec / exec_lo / exec_hi, or a saveexec
    wexec = 0
    for s in kernel_lines(path, name):
        m = re.match(r"^(s_\w+)\s+([\w\[\]:]+)", s)
        if m and (m.group(2).startswith("exec") or "saveexec" in m.group(1)):
            wexec += 1
    print(f"  instructions that write exec {wexec}")
    rep = re.compile(rf"^\s*\.(sgpr_count|vgpr_count|agpr_count|private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count):\s*(\d+)")
    sym, meta = None, collections.OrderedDict()
    for line in open(path, errors="replace"):
        m = re.match(r"^\s*\.name:\s*(\S+)", line)
        if m:
            sym = m.group(1)
        m = rep.match(line)
        if m:
            meta.setdefault(sym, {})[m.group(1)] = int(m.group(2))
        m = re.match(r"^\s*-?\s*\.name:\s*(\S+)", line)
        if m and name in m.group(1):
            sym = m.group(1)
    for k, v in meta.items():
        if k and name in k:
            print(f"  {k}: {v}")


if __name__ == "__main__":
    main()
