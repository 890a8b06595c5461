"""tests/launch_caps.py against the sources it describes: the numbers are read out of csrc/tba_engine.hip and
csrc/k_scan.h as text.  Somebody who retunes a cap meets this test, and changes launch_caps.py with it; the GPU
tests that cross the caps then follow by themselves (they size their inputs from the module)."""
import os
import re

import launch_caps as lc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tombo_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


ENGINE = _src('tba_engine.hip')


def _one(pattern, text=ENGINE):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def _body(start, text=ENGINE):
    """the text from the one line that holds `start` to the first line that is a closing brace in column 0"""
    assert text.count(start) == 1, start
    a = text.index(start)
    return text[a:text.index('\n}', a)]


def test_grid_for():
    blocks_of, cap = _one(r'static unsigned grid_for\(i64 n\) \{ return \(unsigned\)std::min<i64>\(std::max<i64>\('
                          r'\(n \+ 255\) / (\d+), 1\), (\d+)\); \}')
    assert (int(cap), int(blocks_of)) == (lc.GRID_BLOCKS, lc.GRID_THREADS)
    assert lc.GRID_PASS == lc.GRID_BLOCKS * lc.GRID_THREADS
    # every launch through grid_for uses blocks of GRID_THREADS
    launches = re.findall(r'<<<\s*(?:dim3\()?grid_for\([^<>]*?\)(?:, 1\))?, (\d+),', ENGINE)
    assert len(launches) >= 40 and set(launches) == {str(lc.GRID_THREADS)}


def test_classify_launch():
    assert int(_one(r'k_kde_classify<<<grid_for\((\d+) \* n_seg\)')) == lc.WAVE
    assert lc.CLASSIFY_PASS * lc.WAVE == lc.GRID_PASS
    assert 'k_grp_classify<<<grid_for(2 * P.a.n_pos), 256,' in ENGINE


def test_sorter_grids():
    body = _body('static void launch_sort_classes(')
    grids = re.findall(r'(k_grp_sort_\w+)<<<(\d+), (\d+), 0, s>>>', body)
    assert [g[0] for g in grids] == ['k_grp_sort_wave', 'k_grp_sort_wg', 'k_grp_sort_wg']
    assert [(int(b), int(t)) for _, b, t in grids] == [lc.SORT_WAVE_GRID, lc.SORT_LDS_GRID, lc.SORT_GLOBAL_GRID]
    assert lc.SORT_WAVE_PASS == 4096 and lc.SORT_LDS_PASS == 1024 and lc.SORT_GLOBAL_PASS == 256
    group = _src('k_group.h')
    assert 'wave (n <= %d) / workgroup-LDS (n <= %d) / global' % (lc.SORT_WAVE_MAX, lc.SORT_LDS_MAX) in group


def test_block_clamps():
    assert int(_one(r'k_kde_eval<<<dim3\(\(unsigned\)std::min<i64>\(n_seg, (\d+)\)')) == lc.KDE_EVAL_BLOCKS
    step, clamp = _one(r'for \(i64 r0 = 0; r0 < n_reads; r0 \+= (\d+)\)[^\n]*\n\s*k_kd_read_scan<<<dim3\(scan_x, '
                       r'\(unsigned\)std::min<i64>\(n_reads - r0, (\d+)\)\)')
    assert int(step) == int(clamp) == lc.KD_READ_SLICE
    assert int(_one(r'k_kd_seg_means<<<\(unsigned\)std::min<i64>\(\(n_val \+ 63\) / 64, (\d+)\)')) == lc.KD_MEANS_BLOCKS
    assert int(_one(r'k_kd_kmer_means<<<\(unsigned\)std::min<i64>\(n_kmers, (\d+)\)')) == lc.KD_MEANS_BLOCKS


def test_scan_chunk():
    assert int(_one(r'#define SCAN_CHUNK (\d+)\n', _src('k_scan.h'))) == lc.SCAN_CHUNK
    assert 'return (unsigned)((n + SCAN_CHUNK - 1) / SCAN_CHUNK);' in ENGINE


def test_key_partition_rule():
    body = _body('struct KeyPartition {')
    chunks, bits = _one(r'max_chunks = std::max<i64>\(1, std::min<i64>\((\d+), \(\(i64\)1 << (\d+)\) / n_keys\)\);', body)
    assert int(chunks) == lc.PART_MAX_CHUNKS and 1 << int(bits) == lc.PART_MAX_COUNTERS
    least = _one(r'chunk = std::max<i64>\((\d+), \(\(n \+ max_chunks - 1\) / max_chunks \+ 63\) / 64 \* 64\);', body)
    assert int(least) == lc.PART_CHUNK
    assert 'n_chunks = (n + chunk - 1) / chunk;' in body
    assert 'while (((i64)1 << key_bits) < n_keys) key_bits++;' in body
    # the rule as the issue states it, at the sizes the GPU tests use
    assert lc.partition_geometry(9001, 64) == (4096, 3, 6)
    assert lc.partition_geometry(65536, 4 ** 10) == (4096, 16, 20)
    assert lc.partition_geometry(65537, 4 ** 10) == (4160, 16, 20)
    assert lc.partition_geometry(5000, 1 << 24) == (5056, 1, 24)
    assert lc.partition_geometry(4096 * 15 + 1, (1 << 20) + 1)[::2] == (4160, 21)
    assert lc.partition_geometry(1, 1) == (4096, 1, 0)


def test_kmer_dist_rule():
    assert 1 << int(_one(r'#define KD_TABLE_MAX \(\(i64\)1 << (\d+)\)')) == lc.KD_TABLE_MAX
    body = _body('extern "C" int tba_kmer_dist(')
    assert int(_one(r'i64 chunk = (\d+), max_len = 0;', body)) == lc.KD_CHUNK
    assert 'while (chunk < max_len && count_chunks(chunk) > KD_TABLE_MAX / n_kmers) chunk *= 2;' in body
    assert 'if (n_reads > KD_TABLE_MAX / n_kmers)' in body
    assert lc.KD_TABLE_MAX // 4 ** 9 == 512
    assert lc.kmer_dist_geometry([4096 * 510, 5, 9], 9) == (4096, 512)
    assert lc.kmer_dist_geometry([4096 * 510 + 1, 5, 9], 9) == (8192, 258)
    assert lc.kmer_dist_geometry([3, 4000], 1) == (4096, 2)


def test_pass_sample():
    s = lc.pass_sample(lc.GRID_PASS + 1, 5)
    assert s.shape[0] == 2000 + 64 + 64 + 1 and s[0] == 0 and s[-1] == lc.GRID_PASS
    assert lc.pass_sample(65539, 6, pass_len=65535).shape[0] == 2000 + 64 + 64 + 4
    for i in (63, lc.GRID_PASS - 64, lc.GRID_PASS - 1, lc.GRID_PASS):
        assert i in s
    assert (s[1:] > s[:-1]).all()
