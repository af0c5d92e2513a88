# usage (build container): bash tools/build_variants.sh tag1="<src>|<flags>" ...   src = "." (working tree) or a git revision
# Cross-compiles one libfleet_hip.so (and the kernels' code object beside it) per entry into ab_variants/ (git-ignored); a git
# revision is exported to a temporary directory first, so that an older kernel can run beside the tree's on the same box.  Which
# files make a library is the revision's own business: each is built by its own fleetrl_amd/build.py (build_variant).
cd "$(dirname "$0")/.." && mkdir -p ab_variants && rm -f ab_variants/*.so ab_variants/*.hsaco
for spec in "$@"; do
  tag="${spec%%=*}"; rest="${spec#*=}"; src="${rest%%|*}"; flags="${rest#*|}"; [ "$flags" = "$rest" ] && flags=""
  if [ "$src" = "." ]; then dir=.; else dir=$(mktemp -d /tmp/absrc.XXXX); git archive "$src" fleetrl_amd/build.py fleetrl_amd/csrc include | tar -x -C "$dir"; sed -i "s/#define FLEET_ABI_VERSION .*/$(grep '#define FLEET_ABI_VERSION' include/fleet_hip.h)/" "$dir/include/fleet_hip.h"; fi  # (an older revision answers to the tree's ABI number: the public structures have not changed since version 4)
  ( python3 -c 'import runpy, sys; runpy.run_path(sys.argv[1])["build_variant"](sys.argv[2], sys.argv[3].split())' \
      "$dir/fleetrl_amd/build.py" "ab_variants/$tag.so" "$flags" || echo "BUILD FAILED: $tag" ) &
done
wait; ls -la ab_variants
