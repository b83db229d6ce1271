"""Which publishing records the cases of tests/test_peer_minima_hold_gpu.py hold (no GPU): the form with three tables in registers
parks the table of receive 0, keeps those of receives 1 and 2 in their slots and takes the table of receive 3 into the slot of the
parked one — so records with 3 and 4 edges must have each of these receives on side 0 and on side 1 somewhere in the list.  Counted
with ``peer_minima_cases.record_sides`` from the edge lists alone; the colour-major grids are the all-side-1 records."""
import peer_minima_cases as PC

MIXED = ["random-flip 13x11", "thinned 13x11", "bipartite 61+45", "stars 3x4"]
GRIDS = [(4, 5), (5, 5), (13, 11), (40, 36)]


def _cells():
    out = {}
    lists = [PC.record_sides(PC.case(name))[0] for name in MIXED]
    for H, W in GRIDS:                                          # colour-major: no edge is flipped, every publishing record on side 1
        n0, n1, edges = PC.colour_major_graph(H, W)
        pub = [[] for _ in range(n1)]
        for _, b in edges:
            pub[b].append(1)
        lists.append([s for s in pub if s])
    for recs in lists:
        for s in recs:
            assert s == sorted(s) and 1 <= len(s) <= PC.MAX_DEGREE
            for j, side in enumerate(s):
                out[(len(s), j, side)] = out.get((len(s), j, side), 0) + 1
    return out


def test_every_receive_of_three_and_four_edge_records_on_both_sides():
    cells = _cells()
    for edges in (3, 4):
        for j in range(edges):
            for side in (0, 1):
                assert cells.get((edges, j, side), 0) > 0, ("no publishing record with %d edges whose receive %d is on side %d" % (edges, j, side), cells)


def test_records_with_fewer_edges_are_there_too():
    cells = _cells()
    for edges in (1, 2):
        for side in (0, 1):
            assert cells.get((edges, 0, side), 0) > 0, (edges, side, cells)
