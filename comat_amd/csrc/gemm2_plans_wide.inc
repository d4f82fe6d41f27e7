// gemm2_plans_wide.inc - measured plans that choose tile code 14 (128x128, 8 waves, 128-byte k-tiles):
// TUNE_WIDE=1 tools/tune_gemm2.py on an MI355X -> tools/make_gemm2_plans.py --wide.  Same row format as gemm2_plans.inc; plan2
// searches this table first.  A row stands here only where the new shape beat the problem's plan of gemm2_plans.inc by more than
// the spread of the alternating measurement AND cuts k into the same slices as that plan: the results of a launch are then the
// parent plan's bit for bit (tests/test_gemm2_wide_tiles.py holds every row to that).  Three rows the tool wrote, of 1 - 2 calls per
// step each, were taken out by hand: in the step (bench.py --full) they were once not below two runs of the parent by more than
// the difference between those (profiles/gemm2_wide_tiles_shapes.txt).  Trailing comment: us per launch with this plan, with the plan of gemm2_plans.inc, calls per step.
static const Plan2Entry g2_plans_wide[] = {
    {1, 8192, 320, 90, 1, 14, 1},  // 31.8 us (gemm2_plans.inc 34.7), 50 calls
    {1, 512, 1280, 360, 1, 14, 6},  // 31.7 us (gemm2_plans.inc 34.2), 48 calls
    {1, 2048, 640, 180, 1, 14, 3},  // 29.8 us (gemm2_plans.inc 31.7), 42 calls
    {1, 512, 2560, 360, 1, 14, 3},  // 46.5 us (gemm2_plans.inc 52.0), 12 calls
    {1, 512, 1280, 720, 1, 14, 6},  // 48.6 us (gemm2_plans.inc 53.8), 12 calls
    {1, 2048, 640, 540, 1, 14, 3},  // 63.9 us (gemm2_plans.inc 73.6), 6 calls
    {1, 4096, 512, 144, 1, 14, 2},  // 33.6 us (gemm2_plans.inc 36.3), 15 calls
    {1, 2048, 640, 360, 1, 14, 3},  // 46.8 us (gemm2_plans.inc 53.5), 6 calls
    {1, 2048, 1920, 180, 1, 14, 1},  // 58.8 us (gemm2_plans.inc 64.1), 6 calls
    {0, 512, 1408, 40, 3, 14, 1},  // 15.9 us (gemm2_plans.inc 16.9), 30 calls
    {1, 512, 1280, 540, 1, 14, 6},  // 40.1 us (gemm2_plans.inc 44.7), 6 calls
    {0, 8192, 320, 40, 1, 14, 1},  // 18.0 us (gemm2_plans.inc 18.7), 30 calls
    {1, 512, 1920, 360, 1, 14, 4},  // 38.6 us (gemm2_plans.inc 42.2), 6 calls
    {1, 2048, 640, 270, 1, 14, 3},  // 38.3 us (gemm2_plans.inc 41.7), 6 calls
    {1, 2048, 960, 180, 1, 14, 2},  // 38.7 us (gemm2_plans.inc 41.9), 6 calls
    {1, 2048, 640, 90, 1, 14, 3},  // 20.9 us (gemm2_plans.inc 22.1), 6 calls
    {1, 1024, 1280, 360, 1, 14, 3},  // 46.7 us (gemm2_plans.inc 52.3), 1 calls
    {1, 1024, 640, 540, 1, 14, 6},  // 40.1 us (gemm2_plans.inc 45.5), 1 calls
    {0, 256, 10240, 40, 1, 14, 1},  // 16.6 us (gemm2_plans.inc 17.5), 5 calls
    {1, 1024, 1920, 180, 1, 14, 2},  // 37.6 us (gemm2_plans.inc 41.1), 1 calls
    {1, 4096, 960, 90, 1, 14, 1},  // 33.7 us (gemm2_plans.inc 36.4), 1 calls
};
