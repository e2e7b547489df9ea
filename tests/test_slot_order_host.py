"""CPU test of ``difflinker_amd/csrc/slot_order.h``: the header that tells every lane pair of the pair loops which (receiver,
chunk) it walks and every wave how many steps it runs.  A few lines of C++ around the header are compiled with the host compiler
(the header is plain C++ there) and walk every plan: nrec = 1..55 receivers of nb = nrec..110 senders.

* the lanes below nrec g map one-to-one onto the (il, c) pairs, the others get nothing;
* a wave's step count is the largest ``jn`` among its slots (no wave leaves before its longest slot is done, none stays longer);
* the step counts of a plan sum to at most what the receiver-major order ran (active waves times q);
* one workgroup per molecule, n = 35..50: the sums are the table of the change (1009 -> 968 wave-steps);
* whenever the last chunk is as long as the others (r = q) the map is the receiver-major one, slot = il g + c;
* ``slot_div`` (the host's form of it: a division by a float reciprocal) is the integer quotient for every a < 1024, b <= 256.

The receiver-major plan the header is compared with is written out here independently (``old_plan``)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'difflinker_amd', 'csrc')

# n: (q, g, r, wave-steps receiver-major, wave-steps with the short chunks last)
TABLE = {35: (5, 7, 5, 40, 40), 36: (6, 6, 6, 42, 42), 37: (7, 6, 2, 49, 44), 38: (7, 6, 3, 56, 48), 39: (7, 6, 4, 56, 53),
         40: (7, 6, 5, 56, 54), 41: (7, 6, 6, 56, 55), 42: (7, 6, 7, 56, 56), 43: (9, 5, 7, 63, 61), 44: (9, 5, 8, 63, 62),
         45: (9, 5, 9, 72, 72), 46: (10, 5, 6, 80, 72), 47: (10, 5, 7, 80, 74), 48: (10, 5, 8, 80, 76), 49: (10, 5, 9, 80, 79),
         50: (10, 5, 10, 80, 80)}

PROGRAM = r'''
#include <cstdio>
#include <vector>
#include "slot_order.h"

// the receiver-major plan, independently: g = min(256 / nrec, nb) chunks, q = ceil(nb / g) steps, then the fewest chunks
// that need no more steps
static void old_plan(int nrec, int nb, int& g, int& q) {
    g = 256 / nrec < nb ? 256 / nrec : nb;
    q = (nb + g - 1) / g;
    g = (nb + q - 1) / q;
}

int main() {
    long fails = 0, plans = 0, shorter = 0;
    for (int a = 0; a < 1024; ++a)
        for (int b = 1; b <= 256; ++b)
            if (slot_div(a, b) != a / b) { std::printf("FAIL div %d %d\n", a, b); ++fails; }
    for (int nrec = 1; nrec <= 55; ++nrec)
        for (int nb = nrec; nb <= 110; ++nb) {
            int g, q;
            old_plan(nrec, nb, g, q);
            const int r = nb - (g - 1) * q;
            const SlotPlan pl = slot_plan(nrec, nb);
            const SlotOrder so = slot_order(nrec, nb);
            const SlotOrder rm = slot_order(nrec, nb, true);
            ++plans;
            if (pl.g != g || pl.q != q || so.g != g || so.q != q || so.r != r || so.nslots != nrec * g || r < 1 || r > q || nrec * g > NSLOT) {
                std::printf("FAIL plan nrec %d nb %d\n", nrec, nb); ++fails; continue;
            }
            std::vector<int> seen(nrec * g, 0);
            int sum_new = 0, sum_old = 0;
            bool bad = false;
            for (int w = 0; w < SLOT_WAVES; ++w) {
                int longest = 0, longest_rm = 0;
                for (int c = 0; c < 32; ++c) {
                    const int slot = 32 * w + c;
                    const SlotLane sl = slot_lane(so, nb, slot), sr = slot_lane(rm, nb, slot);
                    if (sl.ok != (slot < nrec * g) || sr.ok != sl.ok) bad = true;
                    if (!sl.ok) { if (sl.jn != 0 || sl.il != 0 || sl.c != 0 || sl.j0 != 0) bad = true; continue; }
                    if (sl.il < 0 || sl.il >= nrec || sl.c < 0 || sl.c >= g) { bad = true; continue; }
                    ++seen[sl.il * g + sl.c];
                    // one contiguous range of senders: chunk c starts at c q and has q of them, the last chunk r
                    if (sl.j0 != sl.c * q || sl.jn != (sl.c == g - 1 ? r : q) || sl.j0 + sl.jn > nb) bad = true;
                    if (sl.jn > longest) longest = sl.jn;
                    // the switch of the test-hooks build, and every plan whose last chunk is full: slot = il g + c
                    if (sr.il != slot / g || sr.c != slot % g || sr.j0 != sr.c * q || sr.jn != (sr.c == g - 1 ? r : q)) bad = true;
                    if (r == q && (sl.il != sr.il || sl.c != sr.c || sl.j0 != sr.j0 || sl.jn != sr.jn)) bad = true;
                    if (sr.jn > longest_rm) longest_rm = sr.jn;
                }
                const int steps = slot_wave_steps(so, w), steps_rm = slot_wave_steps(rm, w);
                if (steps != longest) bad = true;
                if (steps_rm != (32 * w < nrec * g ? q : 0) || steps_rm < longest_rm) bad = true;
                sum_new += steps;
                sum_old += steps_rm;
            }
            for (int k = 0; k < nrec * g; ++k) if (seen[k] != 1) bad = true;
            if (sum_new > sum_old) bad = true;
            if (r == q && sum_new != sum_old) bad = true;
            if (sum_new < sum_old) ++shorter;
            if (bad) { std::printf("FAIL map nrec %d nb %d\n", nrec, nb); ++fails; }
            if (nrec == nb && nb >= 35 && nb <= 50) std::printf("TABLE %d %d %d %d %d %d\n", nb, q, g, r, sum_old, sum_new);
            // the other loops of the change: a member of a team of two on 46 atoms, 10 linker receivers of 47 senders
            if ((nrec == 23 && nb == 46) || (nrec == 10 && nb == 47)) std::printf("CASE %d %d %d %d %d %d %d\n", nrec, nb, q, g, r, sum_old, sum_new);
        }
    std::printf("DONE plans %ld fails %ld shorter %ld\n", plans, fails, shorter);
    return 0;
}
'''


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError('no host C++ compiler (c++, g++, clang++ or $CXX)')


@pytest.fixture(scope='module')
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp('slot_order')
    src, exe = d / 'walk.cpp', d / 'walk'
    src.write_text(PROGRAM)
    subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    return out


def test_every_plan_maps_lanes_one_to_one_and_waves_run_their_longest_slot(walk):
    fails = [ln for ln in walk if ln.startswith('FAIL')]
    assert not fails, fails[:10]
    done = walk[-1].split()
    assert done[0] == 'DONE' and int(done[4]) == 0
    assert int(done[2]) == sum(110 - nrec + 1 for nrec in range(1, 56)), 'every nrec in 1..55, nb in nrec..110'
    assert int(done[6]) > 0, 'some plans run fewer wave-steps than before'


def test_wave_steps_of_one_workgroup_per_molecule_are_the_table(walk):
    rows = {int(f[1]): tuple(int(x) for x in f[2:]) for f in (ln.split() for ln in walk if ln.startswith('TABLE'))}
    assert rows == TABLE
    assert sum(v[3] for v in rows.values()) == 1009 and sum(v[4] for v in rows.values()) == 968
    for n, (q, g, r, old, new) in rows.items():
        assert (new == old) == (r == q), n


def test_team_member_and_coordinate_loops_have_one_sender_in_their_last_chunk(walk):
    cases = {(int(f[1]), int(f[2])): tuple(int(x) for x in f[3:]) for f in (ln.split() for ln in walk if ln.startswith('CASE'))}
    # (q, g, r, wave-steps before, after): 230 slots with 207 full chunks, 240 slots with 230 full chunks: the last wave of the
    # first runs one step, the last wave of the second (slots 224 .. 239) still holds six full chunks and runs both
    assert cases[(23, 46)] == (5, 10, 1, 40, 36)
    assert cases[(10, 47)] == (2, 24, 1, 16, 16)
