#!/usr/bin/env python3
"""Byte fixture for the point-set writer, derived from the legacy VTK FORMAT SPECIFICATION ("VTK File Formats", simple legacy
format, dataset POLYDATA) -- not from ir_sgmcmc_amd/utils/imageio.py, which it is there to check.

  vtk_legacy_ascii_points.vtk   part 1 the version line, part 2 a title of at most 256 characters, part 3 ASCII, part 4 DATASET
                                POLYDATA with `POINTS n float` and n coordinate triples, then `VERTICES n size` where size counts
                                every integer of the cell list (n cells of "1 i": size = 2 n), part 5 `POINT_DATA n` with, per
                                array, `SCALARS name float 1`, `LOOKUP_TABLE default` and n values.  Three points, the scalars
                                the trainer writes (tre_of_mean, std_major, pit); the values are short decimals that float32
                                holds exactly, and one pit is a NaN, spelled `nan`.

    python tests/golden/make_landmark_fixtures.py      (no imports but os; rewrites the file under tests/golden/io/)
"""
import os

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'io')

POINTS = [('1.5', '-2.25', '0.125'), ('0', '10', '-0.5'), ('33.75', '4', '1024')]
SCALARS = [('tre_of_mean', ['0.5', '1.25', '3']), ('std_major', ['0.25', '0', '2.5']), ('pit', ['0.75', 'nan', '0.0625'])]
TITLE = 'posterior-mean landmarks (mm)'


def main():
    n = len(POINTS)
    lines = ['# vtk DataFile Version 3.0', TITLE, 'ASCII', 'DATASET POLYDATA', f'POINTS {n} float']
    lines += [' '.join(p) for p in POINTS]
    lines.append(f'VERTICES {n} {2 * n}')
    lines += [f'1 {i}' for i in range(n)]
    lines.append(f'POINT_DATA {n}')
    for name, values in SCALARS:
        lines += [f'SCALARS {name} float 1', 'LOOKUP_TABLE default'] + values
    os.makedirs(HERE, exist_ok=True)
    path = os.path.join(HERE, 'vtk_legacy_ascii_points.vtk')
    with open(path, 'w', newline='\n') as f:
        f.write('\n'.join(lines) + '\n')
    print(os.path.basename(path), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
