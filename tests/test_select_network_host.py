"""The 64-slot selection network of the fast stack kernel (csrc/stack_sort.h, kSelect64: the rows and the columns of the 8 x 8
matrix sorted with the 8-sorter, then a searched post-phase) proved on the host: tools/netsearch/verify_select64.cpp includes
the table itself and checks the 8-sorter on its 2^8 inputs, the post-phase on all 12870 staircase matrices (needed wires 0..4,
29..34, 59..63 in rank order, the two halves of the core on their sides, standard form, nothing lost), and 10^5 float columns
against std::sort - ties across the median window, +-0.0, equal values, +-inf, and a NaN at each of the 64 positions, which must
reach wire 63 under the NaN-propagating maximum."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select64_network_is_proved_on_the_host(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    exe = str(tmp_path / 'verify_select64')
    r = subprocess.run([hipcc, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'astrophotography_amd', 'csrc'),
                        os.path.join(ROOT, 'tools', 'netsearch', 'verify_select64.cpp'), '-o', exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout[-3000:]
    m = re.search(r'select64: (\d+) instructions \(rows 192 \+ columns 192 \+ post-phase (\d+);.* 12870 staircases, (\d+) float columns, (\d+) NaN columns: ok',
                  r.stdout)
    assert m, r.stdout[-3000:]
    total, post, columns, nan_columns = map(int, m.groups())
    assert total == 384 + post
    assert total < 694                                       # the crude bound the search started from; the pruned sorter costs 750
    assert columns == 90000 and nan_columns == 10000         # 10^5 in all, each of the 64 positions held the NaN > 150 times
