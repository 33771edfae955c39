"""The host planners (lotus_amd/csrc/lvs_plan.h, lvs_ivf_plan.h), pinned: dump lines of tests/native/plan_check.cpp recorded from the
commit before each planner got a header of its own (the "ivf", "bucket" and "join" lines: from that commit's arithmetic
copied by hand, see profiles/ivf_plan_refactor_check.md).  A line holds the operand layout, the tile geometry, the two-phase plan, the
route, the chunk list and the workspace offsets of one shape (field order: print_row in plan_check.cpp), so a change of any
planning decision for these shapes shows here - on purpose or not."""
import plan_native

PINS = [
    # a single half-full query tile, k > 1: the 128-query geometry
    "nq=128 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 1 3907 1 0 245 16 10 1 | tp 0 | route 0 0 0 0 0 | chunks 128:0:255 | ws 256 768 2509568 768 2704128 5610240 5643008 | bytes 5643008",
    # ... k = 1 keeps 256 x 256
    "nq=128 nb=1000000 d=768 k=1 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 1 3907 1 0 245 16 1 1 | tp 0 | route 0 0 0 0 0 | chunks 128:0:255 | ws 256 768 251648 768 271104 919296 952064 | bytes 952064",
    # ... and so does the 129th query; lvs_rj_kernel from 129 queries
    "nq=129 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 1 3907 1 0 245 16 10 1 | tp 0 | route 0 0 0 0 0 | chunks 129:1:255 | ws 256 1024 2529536 1024 2725632 5654784 5687808 | bytes 5687808",
    # streaming, one query block
    "nq=1 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 1 3907 1 0 245 16 10 1 | tp 0 | route 2 48 64 1 1 | chunks - | ws 256 512 20224 512 21760 44800 45056 | bytes 45056",
    "nq=2 nb=1000000 d=768 k=56 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 1 3907 1 0 245 16 56 1 | tp 0 | route 2 48 64 1 1 | chunks - | ws 256 512 220160 512 237056 463104 463616 | bytes 463616",
    # streaming, three query blocks of 16 slots
    "nq=96 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 1 3907 1 0 245 16 10 1 | tp 0 | route 2 48 16 3 1 | chunks - | ws 256 768 1882368 768 2028288 4207872 4232448 | bytes 4232448",
    # hi|lo on both sides: three K segments; the streaming kernel would need three sibling groups, so the list kernel
    "nq=96 nb=1000000 d=768 k=10 pack=1/1 hi=0 | lay 768 12 1536 1536 3 36 0 0 768 0 768 0 96 | geo 0 1 3907 1 0 245 16 10 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 768 1882368 768 2028288 4207872 4232448 | bytes 4232448",
    "nq=256 nb=1000000 d=1536 k=10 pack=1/1 hi=0 | lay 1536 24 3072 3072 3 72 0 0 1536 0 1536 0 192 | geo 1 1 3907 1 0 245 16 10 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 1280 5018880 1280 5408000 11220224 11285760 | bytes 11285760",
    # register-resident from 97 queries
    "nq=97 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 1 3907 1 0 245 16 10 1 | tp 0 | route 0 0 0 0 0 | chunks 97:0:255 | ws 256 768 1902080 768 2049536 4252160 4276992 | bytes 4276992",
    # the tail chooser changes the slab count (489 x 8 -> 245 x 16 tiles)
    "nq=256 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 1 3907 1 0 245 16 10 1 | tp 0 | route 0 0 0 0 0 | chunks 256:1:255 | ws 256 1280 5018880 1280 5408000 11220224 11285760 | bytes 11285760",
    # 16 <= k <= 56: the 128-query geometry
    "nq=256 nb=1000000 d=768 k=16 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 2 3907 2 0 127 31 16 1 | tp 0 | route 0 0 0 0 0 | chunks 256:1:255 | ws 256 1280 4162816 1280 8652032 13608192 13673728 | bytes 13673728",
    # k > LVS_RQ_KMAX: list kernel
    "nq=256 nb=1000000 d=768 k=48 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 2 3907 2 0 127 31 48 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 1280 12485888 1280 25953536 39232768 39298304 | bytes 39298304",
    # d = 100 -> 128 halfs: no register-resident shape
    "nq=256 nb=1000000 d=100 k=10 pack=0/0 hi=0 | lay 128 2 128 128 1 2 0 0 0 0 0 0 8 | geo 1 1 3907 1 0 245 16 10 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 1280 5018880 1280 5408000 11220224 11285760 | bytes 11285760",
    # two groups need 2 x 32 768 rows
    "nq=257 nb=65536 d=384 k=10 pack=0/0 hi=0 | lay 384 6 384 384 1 6 0 0 0 0 0 0 24 | geo 1 2 256 2 0 16 16 10 1 | tp 0 | route 0 0 0 0 0 | chunks 257:1:128 | ws 256 1536 330496 1536 5409024 6008576 6025216 | bytes 6025216",
    # 16 groups x 16 ranges, one launch
    "nq=4096 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 16 3907 16 0 48 82 10 1 | tp 0 | route 0 0 0 0 0 | chunks 4096:1:16 | ws 256 16640 15745280 16640 7880960 24002816 25051392 | bytes 25051392",
    # chunked: 4 096 + 1
    "nq=4097 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 17 3907 4 0 119 33 10 1 | tp 0 | route 1 0 0 0 0 | chunks 4096:1:16,1:0:255 | ws 256 16896 39020544 16896 7881984 47279104 48327936 | bytes 48327936",
    # a corpus below LVS_RQ_JOIN_MINROWS: list kernel
    "nq=4097 nb=32767 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 17 128 4 0 8 16 10 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 16896 2639104 16896 7881984 10897664 10897664 | bytes 10897664",
    # nb % 32 != 0: one more list per query from the tail rows
    "nq=8192 nb=250001 d=256 k=15 pack=0/0 hi=0 | lay 256 4 256 256 1 4 0 0 0 0 0 0 16 | geo 1 32 977 32 0 16 62 15 1 | tp 0 | route 1 0 0 0 0 | chunks 8192:1:9 | ws 256 33024 15761664 33024 15761664 32014592 34013440 | bytes 34013440",
    # the headline: 8 x 4 L2 plan with its lead slab; 65 536 + 32 768 + 1 696
    "nq=100000 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 391 3907 8 1 13 301 10 1 | tp 0 | route 1 0 0 0 0 | chunks 65536:2:1,32768:1:2,1696:1:32 | ws 256 400384 104400384 400384 47586304 153945600 157945600 | bytes 157945600",
    "nq=100000 nb=1000000 d=768 k=48 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 782 3907 32 0 7 559 48 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 400384 269200384 400384 400384 269200384 288400384 | bytes 288400384",
    # hi|lo corpus: two K segments, list kernel on the L2 plan
    "nq=100000 nb=1000000 d=768 k=10 pack=1/0 hi=0 | lay 768 12 1536 768 2 24 0 0 0 0 768 0 48 | geo 1 391 3907 8 1 13 301 10 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 400384 104400384 400384 47586304 153945600 157945600 | bytes 157945600",
    # hi_only: one K segment whatever the pack modes
    "nq=100000 nb=1000000 d=768 k=10 pack=1/1 hi=1 | lay 768 12 1536 1536 1 12 0 0 0 0 0 0 48 | geo 1 391 3907 8 1 13 301 10 1 | tp 0 | route 1 0 0 0 0 | chunks 65536:2:1,32768:1:2,1696:1:32 | ws 256 400384 104400384 400384 47586304 153945600 157945600 | bytes 157945600",
    "nq=100000 nb=125000 d=768 k=48 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 782 489 32 0 7 70 48 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 400384 269200384 400384 400384 269200384 269200384 | bytes 269200384",
    "nq=100000 nb=250001 d=768 k=56 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 782 977 32 0 7 140 56 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 400384 314000384 400384 400384 314000384 336400384 | bytes 336400384",
    # short-slab fallback to wide groups
    "nq=20000 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 79 3907 16 0 16 245 10 1 | tp 0 | route 1 0 0 0 0 | chunks 16384:1:4,3616:1:16 | ws 256 80384 25680384 80384 18123264 44625408 45425408 | bytes 45425408",
    # short-slab fallback to wide groups
    "nq=25000 nb=1000000 d=768 k=10 pack=1/0 hi=0 | lay 768 12 1536 768 2 24 0 0 0 0 768 0 48 | geo 1 98 3907 16 0 26 151 10 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 100352 52100352 100352 21343232 74405376 75405568 | bytes 75405568",
    # short-slab fallback to wide groups
    "nq=25000 nb=500000 d=768 k=15 pack=0/1 hi=0 | lay 768 12 768 1536 2 24 0 768 0 0 0 0 96 | geo 1 98 1954 16 0 18 109 15 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 100352 54100480 100352 31964672 87026944 88527104 | bytes 88527104",
    "nq=12500 nb=1000000 d=768 k=48 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 98 3907 16 0 26 151 48 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 50432 124850432 50432 50432 124850432 128050432 | bytes 128050432",
    # 32 768 + 16 384 + 848
    "nq=50000 nb=500000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 196 1954 8 1 9 218 10 1 | tp 0 | route 1 0 0 0 0 | chunks 32768:1:2,16384:1:4,848:1:64 | ws 256 200448 36200448 200448 37443328 75305472 77305600 | bytes 77305600",
    # one solo chunk
    "nq=65536 nb=1000000 d=384 k=2 pack=0/0 hi=0 | lay 384 6 384 384 1 6 0 0 0 0 0 0 24 | geo 1 256 3907 8 1 9 435 2 1 | tp 0 | route 1 0 0 0 0 | chunks 65536:2:1 | ws 256 262400 9699584 262400 9699584 21496064 23593216 | bytes 23593216",
    # 32 768 + 16 384 + 8 192 + 4 096 + the rest
    "nq=65236 nb=10000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 255 39063 8 1 9 4341 10 1 | tp 0 | route 1 0 0 0 0 | chunks 32768:1:2,16384:1:4,8192:1:8,4096:1:16,3796:1:16 | ws 256 261376 47231488 261376 47255296 96575232 113275648 | bytes 113275648",
    "nq=1000000 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 3907 3907 8 1 9 435 10 1 | tp 0 | route 1 0 0 0 0 | chunks 65536:2:1x15,16384:1:4,576:1:80 | ws 256 4000256 724000256 4000256 51186176 773545472 813545472 | bytes 813545472",
    # one slab
    "nq=1000000 nb=10000000 d=64 k=48 pack=0/0 hi=0 | lay 64 1 64 64 1 1 0 0 0 0 0 0 4 | geo 0 7813 39063 32 0 1 39063 48 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 4000256 388000256 4000256 4000256 388000256 644000256 | bytes 644000256",
    # two phases: min_slabs 14
    "nq=100000 nb=1000000 d=768 k=100 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 782 3907 32 0 7 559 56 2 | tp 1 15 512 1 391 3907 32 0 14 280 1 391 3907 8 1 13 301 256 400384 168400384 169200384 169600512 579200512 | route 3 0 0 0 0 | chunks - | ws 256 400384 314000384 400384 400384 358800384 358800384 | bytes 579200512",
    # two phases: the slab cap 273 -> 261 slabs of 15 tiles
    "nq=100000 nb=1000000 d=768 k=2048 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 782 3907 32 0 7 559 56 37 | tp 1 15 4096 1 391 3907 32 0 261 15 1 391 3907 8 1 13 301 256 400384 3132400384 3133200384 3133600512 6410400512 | route 3 0 0 0 0 | chunks - | ws 256 400384 314000384 400384 400384 358800384 358800384 | bytes 6410400512",
    "nq=100000 nb=1000000 d=768 k=57 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 782 3907 32 0 7 559 56 2 | tp 1 15 512 1 391 3907 32 0 11 356 1 391 3907 8 1 13 301 256 400384 132400384 133200384 133600512 543200512 | route 3 0 0 0 0 | chunks - | ws 256 400384 314000384 400384 400384 358800384 358800384 | bytes 543200512",
    "nq=1 nb=10000000 d=8 k=2048 pack=0/0 hi=0 | lay 64 1 64 64 1 1 0 0 0 0 0 0 4 | geo 0 1 39063 1 0 1261 31 56 37 | tp 1 15 4096 1 1 39063 1 0 272 144 1 1 39063 1 0 1261 31 256 512 33280 33536 33792 66560 | route 3 0 0 0 0 | chunks - | ws 256 512 565504 512 512 566016 566016 | bytes 566016",
    # k > 56 without a usable two-phase plan: 18 selection passes
    "nq=4096 nb=4096 d=768 k=1000 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 32 16 32 0 1 16 56 18 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 16640 1851648 16640 16640 3686656 3686656 | bytes 3686656",
    "nq=2 nb=255 d=768 k=57 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 1 1 1 0 1 1 56 2 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 512 1536 512 512 2560 2560 | bytes 2560",
    # two phases beyond 24 GB: selection passes
    "nq=1000000 nb=10000000 d=768 k=1000 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 7813 39063 32 0 1 39063 56 18 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 4000256 452000256 4000256 4000256 900000256 900000256 | bytes 900000256",
    # an empty side
    "nq=0 nb=1000000 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 0 1 3907 1 0 245 16 10 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 256 256 256 21504 24832 25088 | bytes 25088",
    # an empty side
    "nq=100000 nb=0 d=768 k=10 pack=0/0 hi=0 | lay 768 12 768 768 1 12 0 0 0 0 0 0 48 | geo 1 391 1 32 0 1 1 10 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 400384 8400384 400384 47586304 57945600 57945600 | bytes 57945600",
    "nq=0 nb=0 d=8 k=1 pack=0/0 hi=0 | lay 64 1 64 64 1 1 0 0 0 0 0 0 4 | geo 1 1 1 1 0 1 1 1 1 | tp 0 | route 3 0 0 0 0 | chunks - | ws 256 256 256 256 2560 5888 5888 | bytes 5888",
]

# field order: ivf_shape, bucket_shape and join_shape in plan_check.cpp
IVF_PINS = [
    # IVF-Flat: the budget case of tests/ivf_edge_cases.py - 3 001 queries in chunks of 376 and a last one of 369
    "ivf mode=0 nq=3001 nlist=8200 nprobe=2048 d=64 M=1 k=56 pack=0 | rc 0 | chunk 376 tail 369 | lay 3033856 9194240 9194240 15392768 15425792 15555072 3033856 6198528 32265 360536576 | prange 0 0 | bytes 360536576",
    # ... halved once: two chunks of 8 192 and a last chunk of one query
    "ivf mode=0 nq=16385 nlist=4097 nprobe=257 d=1088 M=1 k=16 pack=1 | rc 0 | chunk 8192 tail 1 | lay 7373056 24215808 24215808 36869120 36885760 37165568 7373056 12653312 69890 306649600 | prange 0 0 | bytes 306649600",
    # ... the widest fp16 rows at k = 56, and one K-step beyond: LVS_EUNSUPPORTED
    "ivf mode=0 nq=255 nlist=40 nprobe=4 d=2240 M=1 k=56 pack=0 | rc 0 | chunk 255 tail 0 | lay 2955264 2963456 2963456 2968320 2968576 2969088 2955264 4864 72 3426048 | prange 0 0 | bytes 3426048",
    "ivf mode=0 nq=255 nlist=40 nprobe=4 d=2304 M=1 k=56 pack=0 | rc -4 | bytes -4",
    # nprobe > nlist: LVS_EINVAL
    "ivf mode=0 nq=255 nlist=1 nprobe=16 d=64 M=1 k=16 pack=0 | rc -1 | bytes -1",
    # IVF-SQ8, two-digit bucket sort of the pairs (nlist + 1 > BUCKET_MAX_BINS)
    "ivf mode=1 nq=40000 nlist=24576 nprobe=16 d=2368 M=1 k=56 pack=1 | rc 0 | chunk 16384 tail 7232 | lay 30212352 32309504 32309504 35030016 35128576 35259904 30212352 2720512 32769 152700416 | prange 0 0 | bytes 152700416",
    # IVF-PQ: the tables bound the chunk (10 001 queries at M = 159: 2 501 + ... + 2 498); no tiling regions
    "ivf mode=2 nq=10001 nlist=40 nprobe=4 d=636 M=159 k=56 pack=1 | rc 0 | chunk 2501 tail 2498 | lay 3170304 3250432 410453248 410453248 410453248 410453248 3170304 0 0 414935040 | prange 1 1 | bytes 414935040",
    # ... prange 16 for a full chunk
    "ivf mode=2 nq=40000 nlist=8200 nprobe=2048 d=64 M=8 k=17 pack=0 | rc 0 | chunk 1024 tail 64 | lay 2298112 19075328 27463936 27463936 27463936 27463936 2298112 0 0 312676608 | prange 16 16 | bytes 312676608",
    # the threshold search: no parts region (off_parts = total)
    "ivf mode=3 nq=40000 nlist=4097 nprobe=257 d=1216 M=1 k=0 pack=1 | rc 0 | chunk 16384 tail 7232 | lay 14745856 48431360 48431360 73720832 73737472 74280448 14745856 25289472 135682 74280448 | prange 0 0 | bytes 74280448",
    # the bucket sort: one digit up to 24 575 buckets, two from 24 576
    "bucket n=1000000 k=24575 | ok 1 | 123 1 24576 0 0 0 4294967295 0 | 0 12091392 12097536 16097536 16097536 | bytes 16196096",
    "bucket n=1000000 k=24576 | ok 1 | 123 2 4096 7 0 12 4095 4294967295 | 0 2015232 2016256 6016256 10016256 | bytes 10114816",
    # the threshold join, self-join of 70 001 rows: lvs_rj_kernel on whole blocks from the chunk's first row, the last 17 rows
    # and the chunks left with a short corpus through the list kernel (kernel:c0:cn:r0:rn)
    "join nq=70001 nb=70001 q_row0=0 id_offset=0 d=768 pack=0 metric=0 stride=1 | rj 1 | launches 1:0:32768:0:69984 0:0:32768:69984:17 1:32768:32768:32768:37216 0:32768:32768:69984:17 0:65536:4096:65536:4465 0:69632:369:69632:369",
    # ... a plain join of the same shape
    "join nq=70001 nb=70001 q_row0=-1 id_offset=0 d=768 pack=0 metric=0 stride=1 | rj 1 | launches 1:0:32768:0:69984 0:0:32768:69984:17 1:32768:32768:0:69984 0:32768:32768:69984:17 1:65536:4096:0:69984 0:65536:4096:69984:17 1:69632:369:0:69984 0:69632:369:69984:17",
    # ... queries that are rows 5 000 .. of the corpus
    "join nq=40000 nb=40001 q_row0=5000 id_offset=0 d=768 pack=0 metric=0 stride=1 | rj 1 | launches 1:0:32768:4992:35008 0:0:32768:40000:1 0:32768:4096:37760:2241",
    # ... below 2 048 queries, or hi|lo rows: one launch of the list kernel
    "join nq=2047 nb=100031 q_row0=0 id_offset=0 d=768 pack=0 metric=0 stride=1 | rj 0 | launches 0:0:2047:0:100031",
    "join nq=40000 nb=100000 q_row0=0 id_offset=0 d=768 pack=1 metric=0 stride=1 | rj 0 | launches 0:0:40000:0:100000",
]


def test_pinned_plans():
    out = plan_native.run("--dump")
    assert out.returncode == 0, out.stdout[-500:]
    have = {ln.split("|")[0]: ln for ln in out.stdout.splitlines()}
    assert sum(key.startswith("nq=") for key in have) == 147840
    for pin in PINS + IVF_PINS:
        assert have[pin.split("|")[0]] == pin
