"""The stamps build's side buffer, read from hnsw_rs_amd/csrc/stamp_slots.inc: STRIDE values per query, and per list
(LEAN, MERGE, Q8, FAT, GENERIC, PAIR) the slots' numbers and descriptions by name.
   from stamp_slots import STRIDE, slots, descriptions
   L = slots('LEAN'); D[:, L['TOTAL']]"""
import os
import re

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hnsw_rs_amd', 'csrc', 'stamp_slots.inc')
_X = re.compile(r'^\s*X\(\s*(\w+)\s*,\s*(\w+)\s*,\s*(\d+)\s*,\s*"([^"]*)"\s*\)')


def parse(path=TABLE):
    """(stride, {list: [(name, number, description), ...]}) in the table's order"""
    stride, lists = None, {}
    with open(path) as f:
        for line in f:
            m = re.match(r'#define\s+HX_STAMP_STRIDE\s+(\d+)', line)
            if m:
                stride = int(m.group(1))
            m = _X.match(line)
            if m:
                lists.setdefault(m.group(1), []).append((m.group(2), int(m.group(3)), m.group(4)))
    if stride is None or not lists:
        raise ValueError('no slot table in ' + path)
    return stride, lists


STRIDE, LISTS = parse()


def slots(kernel):
    """name -> number"""
    return {name: number for name, number, _ in LISTS[kernel]}


def descriptions(kernel):
    """number -> description"""
    return {number: desc for _, number, desc in LISTS[kernel]}
